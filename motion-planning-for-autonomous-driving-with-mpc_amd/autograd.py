"""The batched solve as a differentiable layer: x*(p) with gradients to p through the parametric sensitivities of the optimum
(include/mpcgpu.h: mpc_solve_batch_sens_dev, mpc_sens_adjoint_dev).

    from <package>.autograd import MPCSolve
    x, status = MPCSolve.apply(solver, x0, p)           # x0, p: float64 device tensors [B, n_w]; torch's current stream
    loss = f(x); loss.backward()                         # p.grad = (dx*/dp)' dloss/dx

Gradients flow to p only (x0 is the initial guess: at an isolated optimum x* does not depend on it).  The obstacle centres are the solver's
own (its descriptor's): per-instance obstacles (the `obst` argument of solve) are not taken by this layer, and no derivative with respect
to them exists.  Rows whose status is not 1 get NaN
gradients; failed="zero" masks them to 0 instead.  The backward pass differentiates the snapshot the forward solve left in the solver's
handle: any later solve on the same solver makes it raise.
"""
from __future__ import annotations

import torch

from .solver import BatchedMPCSolver


class MPCSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver: BatchedMPCSolver, x0: torch.Tensor, p: torch.Tensor, failed: str = "nan"):
        if failed not in ("nan", "zero"):
            raise ValueError('failed must be "nan" or "zero"')
        for name, t in (("x0", x0), ("p", p)):
            if t.dtype != torch.float64 or not t.is_cuda or t.dim() != 2 or t.shape[1] != solver.n_w:
                raise ValueError(f"{name} must be a float64 device tensor [B, {solver.n_w}]")
        B = x0.shape[0]
        if p.shape[0] != B:
            raise ValueError("x0 and p must have the same number of rows")
        x0c, pc = x0.detach().contiguous(), p.detach().contiguous()
        x = torch.empty_like(x0c)
        status = torch.empty(B, dtype=torch.int32, device=x0.device)
        stream = torch.cuda.current_stream(x0.device).cuda_stream
        ctx.gen = solver.solve_sens_device(B, x0c.data_ptr(), pc.data_ptr(), x.data_ptr(), d_status=status.data_ptr(), stream=stream)
        ctx.solver, ctx.B, ctx.failed = solver, B, failed
        ctx.save_for_backward(status)
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, grad_x, grad_status):
        solver = ctx.solver
        if solver._sens_gen != ctx.gen:
            raise RuntimeError("MPCSolve.backward: the solver has solved again since this forward pass; its snapshot of the final iterates is gone")
        (status,) = ctx.saved_tensors
        seed = grad_x.detach().to(torch.float64).contiguous()
        grad_p = torch.empty_like(seed)
        stream = torch.cuda.current_stream(seed.device).cuda_stream
        solver.sens_adjoint_device(ctx.B, seed.data_ptr(), grad_p.data_ptr(), stream=stream)      # MPC_ERR_STATE after any other solve
        if ctx.failed == "zero":
            grad_p = torch.where((status == 1)[:, None], grad_p, torch.zeros_like(grad_p))
        return None, None, grad_p, None


def mpc_solve(solver: BatchedMPCSolver, x0: torch.Tensor, p: torch.Tensor, failed: str = "nan"):
    """functional form of MPCSolve.apply: (x [B, n_w], status [B] int32)"""
    return MPCSolve.apply(solver, x0, p, failed)
