"""The batched solve as a differentiable layer: x*(p, obst, weights, bounds) with gradients to p, to the obstacle circle centres, to the cost
weights and to the bounds through the parametric sensitivities of the optimum (include/mpcgpu.h: mpc_solve_batch_sens_dev,
mpc_sens_adjoint_dev, mpc_sens_obst_dev, mpc_sens_weights_dev, mpc_sens_bounds_dev).

    from <package>.autograd import MPCSolve
    x, status = MPCSolve.apply(solver, x0, p)           # x0, p: float64 device tensors [B, n_w]; torch's current stream
    loss = f(x); loss.backward()                         # p.grad = (dx*/dp)' dloss/dx

    obst = obstacle_centres(pose, obst_offset)           # pose [B, 3] (x, y, heading) of every instance's obstacle -> [B, 6]
    x, status = mpc_solve(solver, x0, p, obst=obst)      # the solve takes these centres; obst.grad / pose.grad = (dx*/do)' dloss/dx

    wt = torch.tensor(solver.weights, requires_grad=True)   # [7] float64 = [Q_0 .. Q_4 | R_0, R_1], on any device
    x, status = mpc_solve(solver, x0, p, weights=wt)     # sets the solver's weights, then solves; wt.grad = sum over the rows of (dx*/dwt)' dloss/dx

    bv = torch.tensor(solver.bounds_vector(), requires_grad=True)   # [n_b] float64 = [lbx | ubx | fl, fu, ol, ou], on any device
    x, status = mpc_solve(solver, x0, p, bounds=bv)      # sets the solver's bounds, then solves; bv.grad = sum over the rows of (dx*/dbv)' dloss/dx

Gradients flow to p and, when they are given, to obst, weights and bounds (x0 is the initial guess: at an isolated optimum x* does not depend on it).  Without
obst the obstacle centres are the solver's own (its descriptor's) and the layer is what it was before obst existed, bit for bit.  Rows whose
status is not 1 get NaN gradients; failed="zero" masks them to 0 instead.  The backward pass differentiates the snapshot the forward solve
left in the solver's handle: any later solve on the same solver makes it raise.

weights [7] is shared by the batch, as the handle's weights are: the forward pass calls solver.set_weights with it -- the solver KEEPS these
weights afterwards -- and for a device tensor that is one copy of seven doubles to the host, hence a synchronisation of the device.  Its
gradient is the sum over the rows of grad_wt [B, 7]: with failed="zero" rows whose status is not 1 contribute 0, with failed="nan" a single
such row makes the whole sum NaN.  With weights=None the layer does not touch the solver's weights and is what it was before, bit for bit.

bounds [n_b] (BatchedMPCSolver.bounds_vector: the circle radius is its entry ol) is shared by the batch in the same way: the forward pass calls
solver.set_bounds(*solver.unpack_bounds(bounds)) -- the solver KEEPS these bounds afterwards -- which for a device tensor is one copy of n_b
doubles to the host, hence a synchronisation.  Its gradient is the sum over the rows of grad_bv [B, n_b] under the same rule for failed rows;
entries of absent bounds (+-inf) get 0.  With bounds=None the layer does not touch the solver's bounds and is what it was before, bit for bit.

The closed loop as a layer, differentiated as a chain of optima (include/mpcgpu.h: mpc_closed_loop_batch_lin_dev, mpc_loop_adjoint_dev;
DESIGN.md section 7):

    wt = torch.tensor(solver.weights, requires_grad=True)
    traj, ctrl = mpc_closed_loop(solver, init_state, wt, path, orient, vdes, steps, obst_track=track, obst_offset=off)
    loss = g(traj, ctrl); loss.backward()                # init_state.grad [B, 5], wt.grad [7] (summed over the egos), track.grad [B, Lt, 3]

The forward pass calls solver.set_weights(weights) -- the solver KEEPS them -- and runs the loop step by step with the per-step gains; the
backward pass is one reverse sweep over the recorded gains and needs no solve, so later solves on the solver do not disturb it.  vdes and the
path are not differentiated.  An ego with a step whose status is not 1 (NaN gains) gets NaN gradients, and with them wt.grad; failed="zero"
gives such egos zero gradients instead.
"""
from __future__ import annotations

import torch

from .solver import BatchedMPCSolver


def obstacle_centres(pose: torch.Tensor, obst_offset: float) -> torch.Tensor:
    """pose [B, 3] (x, y, heading) -> the six circle centres [B, 6] of the obstacle: the centre, then +- obst_offset along the heading.  The
    closed loop's loop_obstacle_centres (csrc/mpc_closed_loop.h) in torch, so that gradients reach the pose."""
    x, y, th = pose[..., 0], pose[..., 1], pose[..., 2]
    cs, sn = torch.cos(th), torch.sin(th)
    return torch.stack([x, y, x + obst_offset * cs, y + obst_offset * sn, x - obst_offset * cs, y - obst_offset * sn], dim=-1)


class MPCSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver: BatchedMPCSolver, x0: torch.Tensor, p: torch.Tensor, failed: str = "nan", obst: torch.Tensor | None = None,
                weights: torch.Tensor | None = None, bounds: torch.Tensor | None = None):
        if failed not in ("nan", "zero"):
            raise ValueError('failed must be "nan" or "zero"')
        for name, t in (("x0", x0), ("p", p)):
            if t.dtype != torch.float64 or not t.is_cuda or t.dim() != 2 or t.shape[1] != solver.n_w:
                raise ValueError(f"{name} must be a float64 device tensor [B, {solver.n_w}]")
        B = x0.shape[0]
        if p.shape[0] != B:
            raise ValueError("x0 and p must have the same number of rows")
        if obst is not None and (obst.dtype != torch.float64 or not obst.is_cuda or tuple(obst.shape) != (B, 6)):
            raise ValueError("obst must be a float64 device tensor [B, 6]")
        if weights is not None:
            if weights.dtype != torch.float64 or tuple(weights.shape) != (7,):
                raise ValueError("weights must be a float64 tensor [7] = [Q_0 .. Q_4 | R_0, R_1]")
            wt = weights.detach().cpu().numpy()                 # (a device tensor: seven doubles to the host, a synchronisation)
            solver.set_weights(wt[:5], wt[5:])
        if bounds is not None:
            if bounds.dtype != torch.float64 or tuple(bounds.shape) != (solver.n_b,):
                raise ValueError(f"bounds must be a float64 tensor [{solver.n_b}] = [lbx | ubx | fl, fu, ol, ou]")
            solver.set_bounds(*solver.unpack_bounds(bounds.detach().cpu().numpy()))     # (a device tensor: a copy to the host, a synchronisation)
        x0c, pc = x0.detach().contiguous(), p.detach().contiguous()
        oc = None if obst is None else obst.detach().contiguous()
        x = torch.empty_like(x0c)
        status = torch.empty(B, dtype=torch.int32, device=x0.device)
        stream = torch.cuda.current_stream(x0.device).cuda_stream
        ctx.gen = solver.solve_sens_device(B, x0c.data_ptr(), pc.data_ptr(), x.data_ptr(), d_status=status.data_ptr(),
                                           d_obst=0 if oc is None else oc.data_ptr(), stream=stream)
        ctx.solver, ctx.B, ctx.failed, ctx.has_obst, ctx.has_wt = solver, B, failed, obst is not None, weights is not None
        if weights is None:
            ctx.save_for_backward(status)
        else:
            ctx.save_for_backward(status, pc)                   # (the weights' right-hand side reads X_ref: the p rows of the solve)
            ctx.wt_device = weights.device
        ctx.has_bv = bounds is not None
        if bounds is not None:
            ctx.bv_device = bounds.device
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, grad_x, grad_status):
        solver = ctx.solver
        if solver._sens_gen != ctx.gen:
            raise RuntimeError("MPCSolve.backward: the solver has solved again since this forward pass; its snapshot of the final iterates is gone")
        status = ctx.saved_tensors[0]
        seed = grad_x.detach().to(torch.float64).contiguous()
        stream = torch.cuda.current_stream(seed.device).cuda_stream
        grad_p = grad_obst = grad_wt = grad_bv = None
        if not (ctx.has_obst or ctx.has_wt or ctx.has_bv) or ctx.needs_input_grad[2]:
            grad_p = torch.empty_like(seed)
            solver.sens_adjoint_device(ctx.B, seed.data_ptr(), grad_p.data_ptr(), stream=stream)      # MPC_ERR_STATE after any other solve
            if ctx.failed == "zero":
                grad_p = torch.where((status == 1)[:, None], grad_p, torch.zeros_like(grad_p))
        if ctx.has_obst and ctx.needs_input_grad[4]:
            grad_obst = torch.empty((ctx.B, 6), dtype=torch.float64, device=seed.device)
            solver.sens_obst_device(ctx.B, d_seed_w=seed.data_ptr(), d_grad_obst=grad_obst.data_ptr(), stream=stream)
            if ctx.failed == "zero":
                grad_obst = torch.where((status == 1)[:, None], grad_obst, torch.zeros_like(grad_obst))
        if ctx.has_wt and ctx.needs_input_grad[5]:
            rows = torch.empty((ctx.B, 7), dtype=torch.float64, device=seed.device)
            solver.sens_weights_device(ctx.B, ctx.saved_tensors[1].data_ptr(), d_seed_w=seed.data_ptr(), d_grad_wt=rows.data_ptr(), stream=stream)
            if ctx.failed == "zero":
                rows = torch.where((status == 1)[:, None], rows, torch.zeros_like(rows))
            grad_wt = rows.sum(dim=0).to(ctx.wt_device)
        if ctx.has_bv and ctx.needs_input_grad[6]:
            rows = torch.empty((ctx.B, solver.n_b), dtype=torch.float64, device=seed.device)
            solver.sens_bounds_device(ctx.B, d_seed_w=seed.data_ptr(), d_grad_bv=rows.data_ptr(), stream=stream)
            if ctx.failed == "zero":
                rows = torch.where((status == 1)[:, None], rows, torch.zeros_like(rows))
            grad_bv = rows.sum(dim=0).to(ctx.bv_device)
        return None, None, grad_p, None, grad_obst, grad_wt, grad_bv


def mpc_solve(solver: BatchedMPCSolver, x0: torch.Tensor, p: torch.Tensor, failed: str = "nan", obst: torch.Tensor | None = None,
              weights: torch.Tensor | None = None, bounds: torch.Tensor | None = None):
    """functional form of MPCSolve.apply: (x [B, n_w], status [B] int32).  obst [B, 6]: every instance's own obstacle circle centres (see
    obstacle_centres); weights [7] float64 on any device: the cost weights [Q_0 .. Q_4 | R_0, R_1] the solver is set to before it solves;
    bounds [n_b] float64 on any device: the bound vector (BatchedMPCSolver.bounds_vector) the solver is set to before it solves; all three may
    require grad"""
    return MPCSolve.apply(solver, x0, p, failed, obst, weights, bounds)


class MPCClosedLoop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver: BatchedMPCSolver, init_state: torch.Tensor, weights: torch.Tensor, path: torch.Tensor, orient: torch.Tensor, vdes: torch.Tensor,
                steps: int, obst_track: torch.Tensor | None, obst_offset: float, noise_mode: int, sigma: float, seed: int, failed: str):
        if failed not in ("nan", "zero"):
            raise ValueError('failed must be "nan" or "zero"')
        dev = init_state.device
        if init_state.dtype != torch.float64 or not init_state.is_cuda or init_state.dim() != 2 or init_state.shape[1] != 5:
            raise ValueError("init_state must be a float64 device tensor [B, 5]")
        B, L = init_state.shape[0], int(steps)
        if weights.dtype != torch.float64 or tuple(weights.shape) != (7,):
            raise ValueError("weights must be a float64 tensor [7] = [Q_0 .. Q_4 | R_0, R_1]")
        for name, t in (("path", path), ("orient", orient), ("vdes", vdes)):
            if t.dtype != torch.float64 or t.device != dev:
                raise ValueError(f"{name} must be a float64 tensor on init_state's device")
        if path.dim() != 3 or path.shape[0] != B or path.shape[2] != 2 or tuple(orient.shape) != (B, path.shape[1]) or tuple(vdes.shape) != (B,):
            raise ValueError("path must be [B, Lp, 2], orient [B, Lp], vdes [B]")
        Lt = 0
        if obst_track is not None:
            if obst_track.dtype != torch.float64 or obst_track.device != dev or obst_track.dim() != 3 or obst_track.shape[0] != B or obst_track.shape[2] != 3:
                raise ValueError("obst_track must be a float64 tensor [B, Lt, 3] on init_state's device")
            Lt = obst_track.shape[1]
        wt = weights.detach().cpu().numpy()                     # (a device tensor: seven doubles to the host, a synchronisation)
        solver.set_weights(wt[:5], wt[5:])
        ins = [t.detach().contiguous() for t in (init_state, path, orient, vdes)]
        tr = None if obst_track is None else obst_track.detach().contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)       # noqa: E731
        traj, ctrl, kg, wg = new(B, L, 5), new(B, L, 2), new(B, L, 2, 5), new(B, L, 2, 7)
        og = new(B, L, 2, 3) if tr is not None else None
        status = torch.empty((B, L), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        solver.closed_loop_lin_device(B, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), L, path.shape[1], traj.data_ptr(),
                                      ctrl.data_ptr(), d_step_status=status.data_ptr(), noise_mode=noise_mode, sigma=sigma, seed=seed, stream=stream,
                                      d_obst_track=0 if tr is None else tr.data_ptr(), Lt=Lt, obst_offset=obst_offset, d_kgain=kg.data_ptr(),
                                      d_wgain=wg.data_ptr(), d_ogain=0 if og is None else og.data_ptr())
        ctx.solver, ctx.failed, ctx.Lt, ctx.wt_device = solver, failed, Lt, weights.device
        ctx.save_for_backward(*([traj, ctrl, kg, wg] + ([og] if og is not None else [])))
        return traj, ctrl

    @staticmethod
    def backward(ctx, grad_traj, grad_ctrl):
        traj, ctrl, kg, wg = ctx.saved_tensors[:4]
        og = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        B, L = traj.shape[:2]
        dev = traj.device
        st = grad_traj.detach().to(torch.float64).contiguous()
        sc = grad_ctrl.detach().to(torch.float64).contiguous()
        gi = torch.empty((B, 5), dtype=torch.float64, device=dev)
        gw = torch.empty((B, 7), dtype=torch.float64, device=dev)
        gt = torch.empty((B, ctx.Lt, 3), dtype=torch.float64, device=dev) if og is not None else None
        ctx.solver.loop_adjoint_device(B, L, traj.data_ptr(), ctrl.data_ptr(), d_kgain=kg.data_ptr(), d_wgain=wg.data_ptr(), d_ogain=0 if og is None else og.data_ptr(),
                                       Lt=ctx.Lt, d_seed_traj=st.data_ptr(), d_seed_ctrl=sc.data_ptr(), d_grad_init=gi.data_ptr(), d_grad_wt=gw.data_ptr(),
                                       d_grad_track=0 if gt is None else gt.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        if ctx.failed == "zero":
            good = ~torch.isnan(kg).reshape(B, -1).any(dim=1)
            gi = torch.where(good[:, None], gi, torch.zeros_like(gi))
            gw = torch.where(good[:, None], gw, torch.zeros_like(gw))
            if gt is not None:
                gt = torch.where(good[:, None, None], gt, torch.zeros_like(gt))
        return None, gi, gw.sum(dim=0).to(ctx.wt_device), None, None, None, None, gt, None, None, None, None, None


def mpc_closed_loop(solver: BatchedMPCSolver, init_state: torch.Tensor, weights: torch.Tensor, path: torch.Tensor, orient: torch.Tensor, vdes: torch.Tensor,
                    steps: int, obst_track: torch.Tensor | None = None, obst_offset: float = 0.0, noise_mode: int = 0, sigma: float = 0.0, seed: int = 0,
                    failed: str = "nan"):
    """the closed loop of B egos as a differentiable layer: (traj [B, steps, 5], ctrl [B, steps, 2]).  init_state [B, 5], path [B, Lp, 2],
    orient [B, Lp], vdes [B], obst_track [B, Lt, 3] | None: float64 device tensors; weights [7] float64 on any device, which the solver is set
    to before the loop runs.  init_state, weights and obst_track may require grad."""
    return MPCClosedLoop.apply(solver, init_state, weights, path, orient, vdes, steps, obst_track, obst_offset, noise_mode, sigma, seed, failed)
