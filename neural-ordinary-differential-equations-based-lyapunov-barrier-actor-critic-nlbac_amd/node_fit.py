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

And the measurement beside the fit — the prediction error by look-ahead step and state component:

  * ``traj_error_stats(pred, target, x0, valid=None)`` — float64 sums over the valid windows, one
    ``nlbac_traj_err_stats`` call; ``error_report`` turns them into rmse / mae / skill on the host;
  * ``validate_rollout(model, states, controls, solver, time_interval)`` — ``train_rollout_step`` without the optimiser.

``SAC_CBF_CLF.validate_node_windows`` / ``validate_node`` are the same on the agent's model and replay.
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


# ---------------------------------------------------------------------------------------------------------------------
# Validation: the prediction error by look-ahead step and state component
# ---------------------------------------------------------------------------------------------------------------------
STAT_PLANES = ("sse", "sae", "max", "base", "tss")       # nlbac_traj_err_stats: stats [5][H][n_s]
STATS_MAX_NS, STATS_ELEMS, STATS_MAX_BLOCKS = 16, 2048, 128


def stats_blocks(n, n_s):
    """Workgroups per step of ``nlbac_traj_err_stats``: min(128, ceil(n n_s / 2048))."""
    return max(1, min(STATS_MAX_BLOCKS, (n * n_s + STATS_ELEMS - 1) // STATS_ELEMS))


def stats_scratch_doubles(H, n, n_s):
    return H * stats_blocks(n, n_s) * (len(STAT_PLANES) * n_s + 1)


def traj_error_stats_launch(pred, target, x0, valid, H, n, n_s, scratch, stats, nvalid):
    """The two launches of ``nlbac_traj_err_stats`` (device buffers, all contiguous; ``valid`` float 1 / 0 or None)."""
    _lib.call("nlbac_traj_err_stats", pred.data_ptr(), target.data_ptr(), x0.data_ptr(),
              valid.data_ptr() if valid is not None else None, n, H, n_s, scratch.data_ptr(), scratch.numel(),
              stats.data_ptr(), nvalid.data_ptr(), stream_ptr())


def traj_error_stats(pred, target, x0, valid=None):
    """Error statistics of predicted trajectories: ``pred`` / ``target`` (H, B, n_s) and ``x0`` (B, n_s) CUDA float32,
    ``valid`` (B,) (nonzero = the window counts; None = all).  Returns ``(stats, nvalid)`` on the device, without a
    synchronisation: ``stats`` (5, H, n_s) float64 — over the valid windows, with e = pred - target formed in float64,
    the planes ``STAT_PLANES``: sum e^2, sum |e|, max |e|, sum (x0 - target)^2 (the persistence baseline: the state does
    not move) and sum target^2 — and ``nvalid`` () int64, the valid windows.  One ``nlbac_traj_err_stats`` call: float64
    throughout, the same bits on every call, a NaN / Inf error of a valid window shows in its (k, c) entry of the first
    three planes.  ``error_report`` turns the pair into rmse / mae / skill."""
    for name, t in (("pred", pred), ("target", target), ("x0", x0)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != (2 if name == "x0" else 3):
            raise TypeError("traj_error_stats: %s must be a float32 %s tensor"
                            % (name, "(B, n_s)" if name == "x0" else "(H, B, n_s)"))
    if pred.shape != target.shape or pred.numel() == 0:
        raise ValueError("traj_error_stats: pred %s and target %s must have the same non-empty shape"
                         % (tuple(pred.shape), tuple(target.shape)))
    H, n, n_s = pred.shape
    if tuple(x0.shape) != (n, n_s):
        raise ValueError("traj_error_stats: x0 must be (%d, %d); got %s" % (n, n_s, tuple(x0.shape)))
    if n_s > STATS_MAX_NS:
        raise ValueError("traj_error_stats: at most %d state components; got %d" % (STATS_MAX_NS, n_s))
    if valid is not None:
        valid = torch.as_tensor(valid)
        if valid.numel() != n:
            raise ValueError("traj_error_stats: valid must hold one entry per window (%d); got %d" % (n, valid.numel()))
    if pred.device.type != "cuda" or target.device != pred.device or x0.device != pred.device:
        raise ValueError("traj_error_stats: pred, target and x0 must be on the same CUDA device")
    dev = pred.device
    if valid is not None:
        valid = (valid.to(dev).reshape(-1) != 0).to(torch.float32).contiguous()
    scratch = torch.empty(stats_scratch_doubles(H, n, n_s), dtype=torch.float64, device=dev)
    stats = torch.empty(len(STAT_PLANES), H, n_s, dtype=torch.float64, device=dev)
    nvalid = torch.empty((), dtype=torch.int64, device=dev)
    traj_error_stats_launch(pred.detach().contiguous(), target.detach().contiguous(), x0.detach().contiguous(), valid,
                            H, n, n_s, scratch, stats, nvalid)
    return stats, nvalid


def error_report(stats, nvalid, **meta):
    """``traj_error_stats``'s pair on the host as a dict — a pure host function: ``stats`` a (5, H, n_s) CPU tensor (or
    array), ``nvalid`` an int (or a one-element tensor).  With V = nvalid, float64 CPU tensors unless said otherwise:

        windows_valid   V (int)
        rmse  (H, n_s)  sqrt(sse / V)                  mae  (H, n_s)  sae / V            max_abs (H, n_s)
        skill (H, n_s)  1 - sse / base — the share of the persistence baseline's squared error the model removes: 1 a
                        perfect prediction, 0 no better than "the state does not move", negative worse; NaN where
                        base == 0 (that component never moved)
        nrmse (H, n_s)  sqrt(sse / tss)
        rmse_step (H,)  sqrt(sum_c sse / (V n_s))
        mse   (float)   sum_k sum_c sse / (V H n_s) — the fit's own loss (``traj_mse``) on these windows

    With V = 0 every ratio is NaN and nothing raises.  ``meta`` is merged in (it may not reuse a key above)."""
    st = torch.as_tensor(stats).detach().to("cpu", torch.float64)
    if st.dim() != 3 or st.shape[0] != len(STAT_PLANES):
        raise ValueError("error_report: stats must be (5, H, n_s); got %s" % (tuple(st.shape),))
    V = int(nvalid.item()) if isinstance(nvalid, torch.Tensor) else int(nvalid)
    if V < 0:
        raise ValueError("error_report: nvalid must be >= 0; got %d" % V)
    sse, sae, mx, base, tss = st.unbind(0)
    _, H, n_s = st.shape
    Vt = torch.tensor(float(V), dtype=torch.float64)          # (tensor division: 0 / 0 is NaN, nothing raises)
    nan = torch.full_like(sse, float("nan"))
    rep = dict(windows_valid=V, rmse=torch.sqrt(sse / Vt), mae=sae / Vt, max_abs=mx.clone(),
               skill=torch.where(base == 0, nan, 1.0 - sse / base), nrmse=torch.sqrt(sse / tss),
               rmse_step=torch.sqrt(sse.sum(1) / (Vt * n_s)), mse=float(sse.sum() / (Vt * H * n_s)))
    clash = set(rep) & set(meta)
    if clash:
        raise ValueError("error_report: meta may not reuse %s" % ", ".join(sorted(clash)))
    rep.update(meta)
    return rep


def validate_rollout(model, states, controls, solver, time_interval, valid=None, step_size=None, step_control="batch"):
    """How well ``model`` predicts observed trajectories — ``train_rollout_step``'s arguments without the optimiser:
    ``states`` (H+1, B, n_s), ``controls`` (H, B, n_c), ``valid`` (B,) or None.  Under ``torch.no_grad()``:
    ``rollout(model, states[0], controls, time_interval, method=solver, step_size=step_size)``, then
    ``traj_error_stats(out[1:], states[1:], states[0], valid)``; returns its ``error_report`` (host numbers: this call
    waits for the device).  Nothing of the model changes.

    The error is the one the fit's loss minimises (``traj_mse`` on ``state_rows`` outputs): plain differences of the
    state components.  ANGLES ARE NOT WRAPPED — a heading that crosses +-pi between prediction and target counts as an
    error of about 2 pi, here as in the fit.

    ``step_control="tile"`` (dopri5, the control-affine nets the tile kernels serve) is passed on to ``rollout`` with
    ``info={}``; the report gains ``accepted_mean`` / ``accepted_max`` / ``attempts_mean`` / ``attempts_max`` (H,), the
    dopri5 steps of the tiles per interval, reduced on the device — how many steps the field takes on real data.
    ``rollout``'s own refusals propagate unchanged (its ``_check`` runs here first with ``on_device=False``, so that host
    inputs are refused before they are moved); every refusal comes before a device is touched."""
    from .rollout import _check, rollout
    states = torch.as_tensor(states, dtype=torch.float32)
    controls = torch.as_tensor(controls, dtype=torch.float32)
    if states.dim() != 3 or controls.dim() != 3 or states.shape[0] != controls.shape[0] + 1:
        raise ValueError("validate_rollout: states (H+1, B, n_s) and controls (H, B, n_c); got %s and %s"
                         % (tuple(states.shape), tuple(controls.shape)))
    if states.shape[2] > STATS_MAX_NS:
        raise ValueError("validate_rollout: at most %d state components; got %d" % (STATS_MAX_NS, states.shape[2]))
    if valid is not None:
        valid = torch.as_tensor(valid)
        if valid.numel() != states.shape[1]:
            raise ValueError("validate_rollout: valid must hold one entry per window (%d); got %d"
                             % (states.shape[1], valid.numel()))
    dt = float(time_interval)
    info = {} if step_control == "tile" else None
    tile_args = {} if step_control == "batch" else dict(step_control=step_control, info=info)
    _check(model, states[0], controls, dt, solver, step_size, on_device=False, **tile_args)
    dev = model.device_handles()[0].arena.device
    states, controls = states.to(dev), controls.to(dev)
    with torch.no_grad():
        out = rollout(model, states[0], controls, dt, method=solver, step_size=step_size, **tile_args)
        stats, nvalid = traj_error_stats(out[1:], states[1:], states[0], valid)
        steps = None
        if info is not None:
            acc, att = info["accepted"].to(torch.float64), info["attempts"].to(torch.float64)
            steps = torch.stack((acc.mean(0), acc.amax(0), att.mean(0), att.amax(0)))
    meta = {}
    if steps is not None:
        steps = steps.cpu()
        meta = dict(accepted_mean=steps[0], accepted_max=steps[1], attempts_mean=steps[2], attempts_max=steps[3])
    return error_report(stats.cpu(), int(nvalid.cpu()), **meta)
