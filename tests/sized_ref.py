"""Shared by tests/test_sized_cpu.py and tests/test_gpu_solve_sized.py (TEST INFRASTRUCTURE): the NLP with obstacle centres per stage AND a lower
bound per circle row, as a subclass of tests/pred_obst_ref.py's StagedNLP; the radii of the instance families; their reference solutions by the
oracle's dense interior-point method, unchanged, certified with the instance's own bounds."""
import functools

import numpy as np

import pred_obst_ref as ref
from oracle.ipm_numpy import DenseIPM

SEEDS = ref.SEEDS
MIN_CONVERGED = ref.MIN_CONVERGED              # of SEEDS, per (family, N): the cap tests/pred_obst_ref.py uses
FAMILIES = (("lead", 2), ("lead", 3), ("lead", 4), ("lead", 7), ("lead", 10), ("drift", 10))


class SizedNLP(ref.StagedNLP):
    """StagedNLP whose circle rows of stage k, slot j have the lower bound radii[k, j], each three times (the three copies of the row)"""

    def __init__(self, cfg, stages, radii):
        super().__init__(cfg, stages)
        self.radii = np.asarray(radii, dtype=np.float64).reshape(cfg.N + 1, 3)

    def bounds(self):
        lbg, ubg, lbx, ubx = super().bounds()
        lbg = lbg.copy()
        r0 = 1 + self.nx * (self.N + 1)
        lbg[r0:] = np.repeat(self.radii.ravel(), 3)
        return lbg, ubg, lbx, ubx


def radii(family, N, seed, nx=5):
    """[N+1, 3] radius sums of the instance, r = cfg.r_sum the handle's.
    lead, N in {2, 3, 4}: r + U(-0.3, 0.3)[3] 2 ((N - 1) dt)^2 from stage 2 on (no control reaches the position before it);
    lead, N in {7, 10}:   r + U(-0.4, 0.5)[3] from stage (N + 1) // 2 on -- a switch to another obstacle at mid-horizon;
    drift, N = 10:        r + U(-0.4, 0.5)[3] k / N"""
    cfg = ref.cfg_for(N, nx)
    r, k = cfg.r_sum, np.arange(N + 1)[:, None]
    if family == "lead" and N <= 4:
        rng = np.random.default_rng(99500 + 100 * N + seed)
        return r + rng.uniform(-0.3, 0.3, 3)[None, :] * 2.0 * ((N - 1) * cfg.dt) ** 2 * (k >= 2)
    rng = np.random.default_rng(99000 + 100 * N + seed)
    u = rng.uniform(-0.4, 0.5, 3)[None, :]
    if family == "lead":
        return r + u * (k >= (N + 1) // 2)
    return r + u * k / N


def reference_solve(name, N, seed, nx=5):
    """the oracle's dense interior-point method on the sized instance: its optimum [n_w], or None where it does not converge"""
    x0, p, st = ref.instance(name, N, seed, nx)
    r = DenseIPM(SizedNLP(ref.cfg_for(N, nx), st, radii(name, N, seed, nx))).solve(x0, p)
    return r["x"] if r["status"] == 1 else None


@functools.lru_cache(maxsize=None)
def family(name, N, nx=5, n=SEEDS):
    """the instances of (family, N) on which the reference converges on the SIZED problem: dict(x0 [n, n_w], p, stages [n, N+1, 3, 2], radii
    [n, N+1, 3], x_ref, active [n] (a circle row within 1e-6 of its own bound at the optimum), x_equal [n, n_w] (the reference's optimum of
    the same instance with the handle's radius on every row; NaN where that one does not converge), seeds [n], tried); arrays read-only"""
    cfg = ref.cfg_for(N, nx)
    keep = dict(x0=[], p=[], stages=[], radii=[], x_ref=[], active=[], x_equal=[], seeds=[])
    for seed in range(n):
        x0, p, st = ref.instance(name, N, seed, nx)
        rad = radii(name, N, seed, nx)
        x = reference_solve(name, N, seed, nx)
        if x is None:
            continue
        X = x[2 * N:].reshape(N + 1, nx)
        xe = ref.reference_solve(name, N, seed, nx)
        for k_, v in zip(keep, (x0, p, st, rad, x, own_clearance(cfg, X, st, rad).min() <= 1e-6, np.full_like(x, np.nan) if xe is None else xe, seed)):
            keep[k_].append(v)
    out = {key: np.array(v) for key, v in keep.items()}
    for v in out.values():
        v.setflags(write=False)
    out["tried"] = n
    return out


def own_clearance(cfg, X, stages, rad):
    """[N+1, 3] distance of pair (j, j) minus the row's own radius sum: X [N+1, >=5] states, stages [N+1, 3, 2], rad [N+1, 3]"""
    d = []
    for j, sg in enumerate((0.0, 1.0, -1.0)):
        ex = X[:, 0] + sg * cfg.ego_offset * np.cos(X[:, 4])
        ey = X[:, 1] + sg * cfg.ego_offset * np.sin(X[:, 4])
        d.append(np.hypot(ex - stages[:, j, 0], ey - stages[:, j, 1]) - rad[:, j])
    return np.stack(d, axis=1)


def batch(parts):
    """families interleaved into one batch: parts = ((name, N), ...) of one N -> dict(x0, p, stages [B, N+1, 6], radii [B, N+1, 3], x_ref,
    x_equal, active, fam [B] index into parts)"""
    fams = [family(*q) for q in parts]
    rows = sorted((i, f) for f, d in enumerate(fams) for i in range(len(d["x0"])))
    pick = lambda key: np.ascontiguousarray(np.array([fams[f][key][i] for i, f in rows]))      # noqa: E731
    B = len(rows)
    return dict(x0=pick("x0"), p=pick("p"), stages=pick("stages").reshape(B, -1, 6), radii=pick("radii"), x_ref=pick("x_ref"),
                x_equal=pick("x_equal"), active=pick("active"), fam=np.array([f for _, f in rows]))


# ---- the selection of the loop through traffic of mixed sizes, in numpy, without the cull --------------------------------------------------------
def select_sized(i, poses, tracks, offsets, rsums, r_handle, pairing, ego_offset, desc_obst):
    """rows [B,N+1,6], radii [B,N+1,3], chosen [B,N+1,3], margin [B,N+1,3] of the solve of step i: tests/traffic_ref.py's select with every distance
    of obstacle m less delta_m = rsums[m] - r_handle; the slot's radius is the winner's rsums[m], r_handle where nothing is present"""
    import traffic_ref as tref
    B, K = poses.shape[:2]
    tracks, offsets = tref._as4(tracks, offsets, B)
    rs = np.asarray(rsums, dtype=np.float64)
    rs = np.broadcast_to(rs, (B,) + rs.shape) if rs.ndim == 1 else rs
    M, Lt = tracks.shape[1:3]
    rows = np.minimum(i + np.arange(K), Lt - 1)
    D, O = tref.distances(poses, tracks, offsets, rows, ego_offset)
    D = D - (rs - r_handle)[:, None, :, None, None]
    out = np.tile(np.asarray(desc_obst, dtype=np.float64).reshape(3, 2), (B, K, 1, 1))
    rad = np.full((B, K, 3), float(r_handle))
    chosen, margin = np.empty((B, K, 3), np.int64), np.empty((B, K, 3))
    bi, ki = np.meshgrid(np.arange(B), np.arange(K), indexing="ij")
    if pairing == 0:
        score = np.min(np.stack([D[..., j, j] for j in range(3)], -1), -1)
        m, mg = tref._two_smallest(score)
        have = m >= 0
        out[have] = O[bi[have], ki[have], m[have]]
        rad[have] = rs[bi[have], m[have]][:, None]
        chosen[:], margin[:] = m[..., None], mg[..., None]
    else:
        for j in range(3):
            m, mg = tref._two_smallest(D[:, :, :, j, :].reshape(B, K, 3 * M))
            have = m >= 0
            out[bi[have], ki[have], j] = O[bi[have], ki[have], m[have] // 3, m[have] % 3]
            rad[bi[have], ki[have], j] = rs[bi[have], m[have] // 3]
            chosen[..., j], margin[..., j] = np.where(have, m // 3, -1), mg
    return out.reshape(B, K, 6), rad, chosen, margin


def clearance_sized(i, state, tracks, offsets, rsums, ego_offset):
    """(clearance [B], nearest [B], margin [B]) of the states before step i: min over present obstacles and all nine pairs of distance - rsums[m]"""
    import traffic_ref as tref
    state = np.asarray(state, dtype=np.float64)
    B = state.shape[0]
    tracks, offsets = tref._as4(tracks, offsets, B)
    rs = np.asarray(rsums, dtype=np.float64)
    rs = np.broadcast_to(rs, (B,) + rs.shape) if rs.ndim == 1 else rs
    D, _ = tref.distances(state[:, None, [0, 1, 4]], tracks, offsets, np.array([min(i, tracks.shape[2] - 1)]), ego_offset)
    flat = (D - rs[:, None, :, None, None]).reshape(B, -1)
    m, mg = tref._two_smallest(flat)
    return np.where(m >= 0, flat.min(-1), np.inf), np.where(m >= 0, m // 9, -1), mg
