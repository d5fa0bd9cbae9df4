"""The one autograd node of every NODE solve entry (``odeint`` / ``odeint_adjoint``, ``rollout``, ``odeint_grid``,
``odeint_dense`` / ``odeint_dense_adjoint``), and what its solves share.

An entry checks its call, makes a SOLVE object for it and hands it to ``SolveNode.apply(solve, n_in, *inputs, *params)``.
A solve object is made per call, lives as long as the node's ``ctx`` and holds none of the caller's graph tensors.  It has

  ``api``          the entry's name, for the messages;
  ``func``         the model (``param_grads`` cuts the flat gradient along its parameters);
  ``with_params``  whether the solve differentiates the parameters at all (keep mode "params"; an adjoint solve with
                   ``adjoint_params=None``);
  ``saves_out``    True where the backward reads the forward's ``out`` (the continuous adjoints): the node then saves
                   ``out`` as a saved tensor, so that autograd's check against in-place edits covers it, and hands it back;
  ``forward(*inputs) -> out``   on the detached inputs; leaves in ``kept`` what a backward needs, None without gradients;
  ``backward(dout, need_in, need_p)`` resp. ``backward(dout, need_in, need_p, out=out)``
                   ``-> (a gradient per input, ..., the flat parameter gradient or None)``; ``need_in``: which inputs ask
                   (a gradient nobody asked for need not be formed, and the node drops it anyway).

``PackedSolve`` is the base of the solves whose one input is ``y0 = [x | carried columns]``.  ``param_grads`` and the
slab reduction live here so that ``odeint.py`` — which ``ode_traj`` imports — can use them.
"""
import torch

from . import _lib
from .arena import stream_ptr


def _reduce(arena, used):
    flat = torch.empty(arena.n, dtype=torch.float32, device=arena.device)
    _lib.call("nlbac_reduce_slabs", flat.data_ptr(), arena.grad.data_ptr(), used, arena.n, arena.n, stream_ptr())
    return flat


def param_grads(func, flat):
    """The flat arena gradient as one view per parameter, in ``func.parameters()``'s order."""
    arena = func.device_handles()[0].arena
    return [flat[arena.offset_of[id(p)]:arena.offset_of[id(p)] + p.numel()].view(p.shape) for p in func.parameters()]


class SolveNode(torch.autograd.Function):
    """``apply(solve, n_in, *inputs, *params)``: the arguments' positions are counted here and nowhere else."""

    @staticmethod
    def forward(ctx, solve, n_in, *args):
        ctx.solve, ctx.n_in, ctx.n_params = solve, n_in, len(args) - n_in
        out = solve.forward(*[a.detach() for a in args[:n_in]])
        if solve.saves_out and solve.kept is not None:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, dout):
        solve, first_p = ctx.solve, 2 + ctx.n_in
        assert solve.kept is not None, "%s: nothing was kept for a backward (the forward ran without gradients)" % solve.api
        need_in = ctx.needs_input_grad[2:first_p]
        need_p = solve.with_params and any(ctx.needs_input_grad[first_p:])
        if solve.saves_out:
            out, = ctx.saved_tensors
            *gin, flat = solve.backward(dout.float(), need_in, need_p, out=out)
        else:
            *gin, flat = solve.backward(dout.float(), need_in, need_p)
        gp = param_grads(solve.func, flat) if need_p else [None] * ctx.n_params
        return (None, None, *[g if need else None for g, need in zip(gin, need_in)], *gp)


class PackedSolve:
    """A solve of the packed layout: one input ``y0 = [x | carried columns]`` (n, n_s + n_c), ``out`` (n_out + 1, n,
    n_s + n_c) with ``out[0] = y0`` and the carried columns copied to every output point.  A subclass sets ``n_out`` and
    has ``solve(x0, c, xs)``, which fills ``xs`` (n_out, n, n_s) and leaves ``kept``; its ``backward`` forms the
    gradient of ``y0`` with ``grad_y0``."""
    saves_out = False
    dx0_total = False      # (a packed solve that is its own kept object: ``grad_y0``)

    def __init__(self, func):
        self.func, self.ns, self.kept = func, func.n_s, None

    def split(self, y0):
        y0 = y0.contiguous()
        return y0, y0[:, :self.ns].contiguous(), y0[:, self.ns:].contiguous()

    def forward(self, y0):
        y0, x0, c = self.split(y0)
        n, ns = y0.shape[0], self.ns
        xs = torch.empty(self.n_out, n, ns, dtype=torch.float32, device=y0.device)      # the states at the output points
        self.solve(x0, c, xs)
        out = torch.empty(self.n_out + 1, n, y0.shape[1], dtype=torch.float32, device=y0.device)
        out[0].copy_(y0)
        out[1:, :, :ns].copy_(xs)
        out[1:, :, ns:].copy_(self.carried(xs, c))
        return out

    def carried(self, xs, c):
        """What goes into the carried columns of the outputs 1 .. n_out: the same at every output point."""
        return c

    def grad_y0(self, dout, dx0, dc, copied, kept):
        """d/dy0 from ``out[0]``'s share ``dout[0]``, the solve's own ``dx0`` and ``dc``, and ``copied``: the summed
        share of the output points the carried columns were copied to.  ``kept.dx0_total`` says which of the two
        groupings the solve needs: the time-grid family (``ode_traj``'s kept objects) takes all of ``dout`` and returns
        ``dx0`` with ``dout[0]`` inside; the dense family and ``odeint`` take ``dout[1:]`` and add ``dout[0]`` here, in
        one full-width add.  (On the carried columns both are dout[0] + (dc + copied).)"""
        if kept.dx0_total:
            return torch.cat([dx0, dout[0][:, self.ns:] + (dc + copied)], dim=1)
        return dout[0] + torch.cat([dx0, dc + copied], dim=1)
