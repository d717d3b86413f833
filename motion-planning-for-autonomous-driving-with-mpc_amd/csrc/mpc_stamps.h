// mpc_stamps.h -- the profiling stamps of option timing: a stamped kernel writes the shader clock into slots of its workgroup's row of
// STAMP_SLOTS words; the host prints the mean ticks between two slots under a label (tools/*_timing.py read that text).  One place for
// the slots of every kernel, the (from, to, label) spans of every report and the formatters -- plain C++ over host rows, shared with the
// CPU harness (tests/test_stamp_report.py).
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

namespace mpc {
constexpr int STAMP_SLOTS = 16;
// slot `slot` of row `row` of the stamp buffer `dbg` (null: no stamps), by the thread(s) `pred` holds for
#define MPC_STAMP(dbg, row, slot, pred) do { if ((dbg) && (pred)) (dbg)[(row) * STAMP_SLOTS + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)

enum StageStamp { SB_ENTER, SB_ISSUED, SB_LOADED, SB_P1, SB_RED1, SB_LS, SB_UPDATE, SB_XCHG, SB_EVAL, SB_RED3, SB_END };      // stage_block, wg_stage
enum RicStamp { RT_BEGIN, RT_BWD_END, RT_FWD_END, RT_B15_WAIT, RT_B15_GO, RT_B15_END, RT_F15_WAIT, RT_F15_GO, RT_F15_END, RT_F0 };    // riccati_tile (stage 15 of both sweeps, stage 0 of the forward one)
enum PipeStamp { PW_TAKE = 11, PW_GOT, PW_BCAST, PW_DONE, PW_SIGNALLED,     // k_pipeline: a stage worker's item around stage_block's slots ...
                 PR_WAIT = 11, PR_SWEEP, PR_PUBLISHED };                    // ... a Riccati worker's pass around riccati_tile's
enum WgStamp { WG_ROUND = 12, WG_RECORDS, WG_SWEPT, WG_ROUND_END };         // k_solve_wg: a round around wg_stage's slots
enum StartStamp { PP_BOUNDS = 1, PP_DEFECTS, PP_SCAN1, PP_SCAN2, PP_SCAN3, PP_SUMS,      // prestart_par_block ...
                  KS_BEGIN = 11, KS_ROWS, KS_STORED, KS_SAFE, KS_FENCED };               // ... inside k_start, in front of stage_block<INIT> (SB_ENTER, SB_XCHG ... SB_END)

struct StampSpan { int from, to; const char* label; };
constexpr StampSpan START_SPANS[] = {
    {KS_BEGIN, KS_ROWS, "rows->LDS"}, {KS_ROWS, KS_STORED, "Z/REF stores"}, {KS_STORED, PP_BOUNDS, "bounds+a0"}, {PP_BOUNDS, PP_DEFECTS, "defects"}, {PP_DEFECTS, PP_SCAN1, "scan1"},
    {PP_SCAN1, PP_SCAN2, "tan+scan2"}, {PP_SCAN2, PP_SCAN3, "sincos+scan3"}, {PP_SCAN3, PP_SUMS, "ROLL+sums"}, {PP_SUMS, KS_SAFE, "decide"}, {KS_SAFE, KS_FENCED, "fence"},
    {KS_FENCED, SB_ENTER, "enter"}, {SB_ENTER, SB_XCHG, "init point+exchange"}, {SB_XCHG, SB_EVAL, "eval+assemble"}, {SB_EVAL, SB_RED3, "reduce"}, {SB_RED3, SB_END, "finish"}};
constexpr StampSpan WG_SPANS[] = {
    {WG_ROUND, WG_RECORDS, "records"}, {WG_RECORDS, WG_SWEPT, "sweeps"}, {WG_SWEPT, SB_ENTER, "enter"}, {SB_ENTER, SB_ISSUED, "load+premath"}, {SB_ISSUED, SB_LOADED, "or"}, {SB_LOADED, SB_P1, "P1"},
    {SB_P1, SB_RED1, "reduce1+ls-begin"}, {SB_RED1, SB_LS, "linesearch"}, {SB_LS, SB_UPDATE, "P3-update"}, {SB_UPDATE, SB_XCHG, "exchange"}, {SB_XCHG, SB_EVAL, "P4-eval"},
    {SB_EVAL, SB_RED3, "reduce3"}, {SB_RED3, SB_END, "P5"}, {SB_END, WG_ROUND_END, "drain"}};
constexpr StampSpan STAGE_SPANS[] = {
    {SB_ENTER, SB_ISSUED, "issue-loads"}, {SB_ISSUED, SB_LOADED, "wait+barrier"}, {SB_LOADED, SB_P1, "P1"}, {SB_P1, SB_RED1, "reduce1"}, {SB_RED1, SB_LS, "linesearch"},
    {SB_LS, SB_UPDATE, "P3-update"}, {SB_UPDATE, SB_XCHG, "exchange"}, {SB_XCHG, SB_EVAL, "P4-eval"}, {SB_EVAL, SB_RED3, "reduce3"}, {SB_RED3, SB_END, "P5"}};
constexpr StampSpan PIPE_STAGE_SPANS[] = {
    {PW_TAKE, PW_GOT, "dequeue"}, {PW_GOT, PW_BCAST, "acquire+bcast"}, {PW_BCAST, SB_ENTER, "enter"}, STAGE_SPANS[0], STAGE_SPANS[1], STAGE_SPANS[2], STAGE_SPANS[3], STAGE_SPANS[4], STAGE_SPANS[5],
    STAGE_SPANS[6], STAGE_SPANS[7], STAGE_SPANS[8], STAGE_SPANS[9], {SB_END, PW_DONE, "drain"}, {PW_DONE, PW_SIGNALLED, "signal"}};
// (the labels of the Riccati spans are part of the sentences the reports print them in)
constexpr StampSpan PIPE_RIC_SPANS[] = {
    {PR_WAIT, PR_SWEEP, "wait"}, {PR_SWEEP, RT_BWD_END, "backward"}, {RT_BWD_END, RT_FWD_END, "forward"}, {RT_FWD_END, PR_PUBLISHED, "publish"}, {RT_B15_WAIT, RT_B15_GO, "barrier"},
    {RT_B15_GO, RT_B15_END, "step"}, {RT_F15_WAIT, RT_F15_GO, "barrier"}, {RT_F15_GO, RT_F15_END, "step"}, {RT_BWD_END, RT_F0, "first forward stage"}};
constexpr StampSpan RIC_SPANS[] = {
    {RT_BEGIN, RT_BWD_END, "backward"}, {RT_BWD_END, RT_FWD_END, "forward"}, {RT_B15_WAIT, RT_B15_GO, "bwd barrier-wait"}, {RT_B15_GO, RT_B15_END, "compute"},
    {RT_F15_WAIT, RT_F15_GO, "fwd barrier-wait"}, {RT_F15_GO, RT_F15_END, "compute"}};

inline void appendf(std::string& s, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s += buf;
}
// the spans of `sp` summed over the rows `ran` holds for (a kernel that left early, or in another role, has not stamped them); returns their number
// (WRAP: the difference as the unsigned number it is computed in, else as a signed one)
template <bool WRAP = false, size_t N, class Ran>
int span_sums(const unsigned long long* rows, int nrows, const StampSpan (&sp)[N], double (&acc)[N], Ran ran) {
    int cnt = 0;
    for (double& a : acc) a = 0.0;
    for (const unsigned long long* r = rows; r < rows + (size_t)nrows * STAMP_SLOTS; r += STAMP_SLOTS) {
        if (!ran(r)) continue;
        for (size_t q = 0; q < N; ++q) acc[q] += WRAP ? (double)(r[sp[q].to] - r[sp[q].from]) : (double)(long long)(r[sp[q].to] - r[sp[q].from]);
        ++cnt;
    }
    return cnt;
}
// `head` (with the number of rows counted) and " label=mean" per span
template <bool WRAP = false, size_t N, class Ran>
std::string span_means(const char* head, const unsigned long long* rows, int nrows, const StampSpan (&sp)[N], Ran ran) {
    double acc[N];
    const int cnt = span_sums<WRAP>(rows, nrows, sp, acc, ran);
    std::string s;
    appendf(s, head, cnt);
    for (size_t q = 0; q < N; ++q) appendf(s, " %s=%.0f", sp[q].label, cnt ? acc[q] / cnt : 0.0);
    return s;
}
// k_start: every workgroup
inline std::string format_start_timing(const unsigned long long* rows, int nblk) {
    unsigned long long t0 = ~0ull, t1 = 0ull;
    for (int b = 0; b < nblk; ++b) { t0 = std::min(t0, rows[b * STAMP_SLOTS + KS_BEGIN]); t1 = std::max(t1, rows[b * STAMP_SLOTS + SB_END]); }
    std::string s = span_means("[mpcgpu k_start timing, shader-clock ticks, mean over %d workgroups]", rows, nblk, START_SPANS, [](const unsigned long long*) { return true; });
    appendf(s, "; first start to last end %.0f\n", (double)(t1 - t0));
    return s;
}
// k_solve_wg alone: the third round of every workgroup that had one
inline std::string format_wg_timing(const unsigned long long* rows, int nblk) {
    return span_means("[mpcgpu k_solve_wg timing, shader-clock ticks, third round of %d workgroups]", rows, nblk, WG_SPANS,
                      [](const unsigned long long* r) { return r[WG_ROUND_END] && r[SB_END]; }) + "\n";
}
// k_pipeline: the sixth work item of every stage worker, the sixth pass of every Riccati worker
inline std::string format_pipe_timing(const unsigned long long* rows, int n_wg) {
    auto stage = [](const unsigned long long* r) { return r[PW_SIGNALLED] && r[SB_END]; };
    std::string s = span_means("[mpcgpu pipeline timing, shader-clock ticks, last item of %d stage workers]", rows, n_wg, PIPE_STAGE_SPANS, stage);
    double ra[9];
    const int nr = span_sums(rows, n_wg, PIPE_RIC_SPANS, ra, [&](const unsigned long long* r) { return !stage(r) && r[PR_PUBLISHED] && r[RT_FWD_END]; });
    for (double& v : ra) v = nr ? v / nr : 0.0;
    appendf(s, "\n[last pass of %d Riccati workers] wait=%.0f backward=%.0f forward=%.0f publish=%.0f; stage 15 of the backward sweep: barrier=%.0f step=%.0f, of the forward sweep: barrier=%.0f step=%.0f, its first stage starts %.0f ticks after the backward sweep\n",
            nr, ra[0], ra[1], ra[2], ra[3], ra[4], ra[5], ra[6], ra[7], ra[8]);
    return s;
}
// one launch per kernel: the stage kernel's rows (one per block), and from word 8 * nblk of the same buffer the Riccati kernel's (one per tile)
inline std::string format_stage_timing(const unsigned long long* rows, int nblk, int ntiles) {
    std::string s = span_means<true>("[mpcgpu stage timing, shader-clock ticks per block, mean over %d blocks]", rows, nblk, STAGE_SPANS,
                                     [](const unsigned long long* r) { return r[SB_END] != 0; }) + "\n";
    const unsigned long long* rr = rows + (size_t)8 * nblk;
    const int nt = std::min(ntiles, nblk / 2);          // (the tiles whose rows the buffer holds)
    auto ran = [](const unsigned long long* r) { return r[RT_FWD_END] != 0; };
    auto tile0 = [&](int q) { return (long long)(rr[RIC_SPANS[q].to] - rr[RIC_SPANS[q].from]); };
    if (nt > 0 && ran(rr))
        appendf(s, "[riccati stage 15 of tile 0] bwd barrier-wait=%lld compute=%lld | fwd barrier-wait=%lld compute=%lld\n", tile0(2), tile0(3), tile0(4), tile0(5));
    double ric[6];
    const int c2 = span_sums<true>(rr, nt, RIC_SPANS, ric, ran);
    appendf(s, "[mpcgpu riccati timing, ticks per workgroup, mean over %d] backward=%.0f forward=%.0f\n", c2, c2 ? ric[0] / c2 : 0.0, c2 ? ric[1] / c2 : 0.0);
    return s;
}
// k_solve_wg (option wg_trace): every workgroup leaves [start, end (100 MHz wall clock), rounds, instance-rounds | take-over << 16 | first round << 40]: when did the long ones start?
inline std::string format_wg_trace(const unsigned long long* hw, int n_wtrace) {
    unsigned long long t0 = ~0ull, t1 = 0ull;
    std::vector<int> live;
    for (int w = 0; w < n_wtrace; ++w) if (hw[4 * w + 2]) { t0 = std::min(t0, hw[4 * w]); t1 = std::max(t1, hw[4 * w + 1]); live.push_back(w); }
    std::string s;
    if (live.empty()) return s;
    std::sort(live.begin(), live.end(), [&](int a, int b) { return hw[4 * a + 1] > hw[4 * b + 1]; });
    int late = 0;
    double start_max = 0;
    for (int w : live) { const double st = (double)(hw[4 * w] - t0) * 1e-2; if (st > 5.0) ++late; start_max = std::max(start_max, st); }
    appendf(s, "[mpcgpu wg_trace] %d workgroups with work of %d; span %.1f us; %d of them start more than 5 us after the first (latest start %.1f us); the last to finish:\n",
            (int)live.size(), n_wtrace, (double)(t1 - t0) * 1e-2, late, start_max);
    for (size_t i = 0; i < live.size() && i < 12; ++i) {
        const int w = live[i];
        const double st = (double)(hw[4 * w] - t0) * 1e-2, en = (double)(hw[4 * w + 1] - t0) * 1e-2;
        const double tf = (double)((hw[4 * w + 3] >> 16) & 0xFFFFFFull) * 1e-2, tr1 = (double)((hw[4 * w + 3] >> 40) & 0xFFFFFFull) * 1e-2;
        appendf(s, "    workgroup %5d: start %6.1f us  end %6.1f us  rounds %2d  instance-rounds %2d  -> %.1f us per round; instances taken over after %.1f us, first round done after %.1f us, later rounds %.1f us each\n",
                w, st, en, (int)hw[4 * w + 2], (int)(hw[4 * w + 3] & 0xFFFFu), (en - st) / (double)hw[4 * w + 2], tf, tr1, hw[4 * w + 2] > 1 ? (en - st - tr1) / (double)(hw[4 * w + 2] - 1) : 0.0);
    }
    return s;
}

}  // namespace mpc
