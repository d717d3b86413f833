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
