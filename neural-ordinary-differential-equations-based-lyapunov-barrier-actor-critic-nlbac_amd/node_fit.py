"""Multi-step NODE regression: the loss over a predicted trajectory and one optimiser step on it.

The reference's ``train_step(..., horizon, ...)`` reads ``T = horizon`` and never loops over it (U/sac_cbf_clf/model.py:221-260):
the model is regressed on one-step error only, while every controller update differentiates predictions two
(SimulatedCars) or three (Pvtol) steps ahead.  Here the loop exists:

  * ``traj_mse(pred, target, valid=None)`` — masked MSE over (H, B, n_s) trajectories, one ``nlbac_traj_mse_fwd_bwd``
    launch that also leaves d loss / d pred;
  * ``train_rollout_step(model, states, controls, optimizer, solver, time_interval)`` — ``rollout`` H intervals from
    ``states[0]``, ``traj_mse`` against ``states[1:]``, backward through the whole horizon, ``optimizer.step()``.

``SAC_CBF_CLF.fit_node_windows`` is the same step on the agent's own arena and optimiser kernel, fed by
``DeviceReplayMemory.sample_windows``.
"""
import torch

from . import _lib
from .arena import stream_ptr

LOSS_ELEMS, LOSS_MAX_BLOCKS = 1024, 256      # nlbac_traj_mse_fwd_bwd: partials are [min(256, ceil(H n n_s / 1024))]


def node_fit_options(args):
    """(node_horizon, node_stride) of an agent's ``args``: consecutive transitions per trajectory window of the NODE fit
    (default 1: the reference's one-step fit) and replay rows between them (default 1)."""
    horizon, stride = int(getattr(args, "node_horizon", 1)), int(getattr(args, "node_stride", 1))
    if horizon < 1 or stride < 1:
        raise ValueError("node_horizon and node_stride must be >= 1; got %d and %d" % (horizon, stride))
    return horizon, stride


def loss_blocks(H, n, n_s):
    return min(LOSS_MAX_BLOCKS, (H * n * n_s + LOSS_ELEMS - 1) // LOSS_ELEMS)


def valid_counts(valid, n, device):
    """``valid`` (n,) as the float 1 / 0 device vector the loss kernel reads, and its int32 sums per block of 256
    windows (what ``nlbac_gather_windows`` leaves beside a ``valid`` it produced itself)."""
    v = (torch.as_tensor(valid).to(device).reshape(-1) != 0).to(torch.float32).contiguous()
    if v.numel() != n:
        raise ValueError("valid must hold one entry per window (%d); got %d" % (n, v.numel()))
    nblk = (n + 255) // 256
    pad = torch.zeros(nblk * 256, dtype=torch.float32, device=device)
    pad[:n] = v
    return v, pad.view(nblk, 256).sum(1).to(torch.int32).contiguous()


def traj_mse_launch(pred, target, valid, counts, H, n, n_s, dpred, part, out_ptr):
    """The loss launch and the sum of its partials into the float at ``out_ptr`` (device buffers, all contiguous)."""
    s = stream_ptr()
    nblk = loss_blocks(H, n, n_s)
    assert part.numel() >= nblk
    _lib.call("nlbac_traj_mse_fwd_bwd", pred.data_ptr(), target.data_ptr(),
              valid.data_ptr() if valid is not None else None, counts.data_ptr() if valid is not None else None,
              (n + 255) // 256 if valid is not None else 0, n, H, n_s, dpred.data_ptr(), part.data_ptr(), s)
    _lib.call("nlbac_sum_partials", part.data_ptr(), nblk, 1, 1.0, out_ptr, s)


class _TrajMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, valid):
        H, n, n_s = pred.shape
        p = pred.detach().contiguous()
        t = target.detach().contiguous()
        counts = None
        if valid is not None:
            valid, counts = valid_counts(valid, n, p.device)
        dpred = torch.empty_like(p)
        part = torch.empty(loss_blocks(H, n, n_s), dtype=torch.float32, device=p.device)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        traj_mse_launch(p, t, valid, counts, H, n, n_s, dpred, part, loss.data_ptr())
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None


def traj_mse(pred, target, valid=None):
    """Masked mean squared error over trajectories: ``pred`` / ``target`` (H, B, n_s) CUDA float32, ``valid`` (B,)
    (nonzero = the window counts; None = all).  With V = max(1, number of valid windows)

        loss = sum_i valid_i sum_k sum_c (pred - target)^2 / (V H n_s)

    — ``nn.MSELoss()`` for H = 1 and every window valid.  Scalar tensor; differentiable w.r.t. ``pred`` only."""
    for name, t in (("pred", pred), ("target", target)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3:
            raise TypeError("traj_mse: %s must be a float32 (H, B, n_s) tensor" % name)
    if pred.shape != target.shape or pred.numel() == 0:
        raise ValueError("traj_mse: pred %s and target %s must have the same non-empty shape"
                         % (tuple(pred.shape), tuple(target.shape)))
    if pred.device.type != "cuda" or target.device != pred.device:
        raise ValueError("traj_mse: pred and target must be on the same CUDA device")
    return _TrajMSE.apply(pred, target, valid)


def train_rollout_step(model, states, controls, optimizer, solver, time_interval, valid=None, step_size=None) -> float:
    """One optimiser step of the multi-step NODE regression: ``states`` (H+1, B, n_s) the observed trajectory,
    ``controls`` (H, B, n_c) the control of every interval (the single-net form's time column included, as in
    ``rollout``); predicts ``rollout(model, states[0], controls, time_interval, method=solver)`` and regresses
    ``out[1:]`` on ``states[1:]`` with ``traj_mse`` (windows with ``valid`` 0 do not count).  Any ``torch.optim``
    optimiser over ``model.parameters()``; returns the loss.  ``train_step`` is the reference's one-step form."""
    from .rollout import rollout
    dev = model.device_handles()[0].arena.device
    states = torch.as_tensor(states, dtype=torch.float32).to(dev)
    controls = torch.as_tensor(controls, dtype=torch.float32).to(dev)
    if states.dim() != 3 or controls.dim() != 3 or states.shape[0] != controls.shape[0] + 1:
        raise ValueError("train_rollout_step: states (H+1, B, n_s) and controls (H, B, n_c); got %s and %s"
                         % (tuple(states.shape), tuple(controls.shape)))
    model.train()
    optimizer.zero_grad()
    out = rollout(model, states[0], controls, float(time_interval), method=solver, step_size=step_size)
    loss = traj_mse(out[1:], states[1:], valid)
    loss.backward()
    optimizer.step()
    model.refresh_device_weights()
    return float(loss.item())
