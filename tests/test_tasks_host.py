"""CPU: what each task of ``TASKS`` tells the shared update — the class-level facts (controllers, noise draws, schedules,
NODE-fit buffers) and every launch descriptor its ``value_now_io`` / ``extra_value_io`` / ``plan`` fill in, resolved to
the workspace buffer (name + byte offset) each pointer lands in.  The tables below are literal: a change of the task
classes that moves a pointer, a width, a stride, an array or a schedule shows up here.  No kernel is launched."""
from types import SimpleNamespace as NS

import pytest
import torch

import nlbac_amd  # noqa: F401
from nlbac_amd import _lib
from nlbac_amd.sac_cbf_clf import tasks, update_plan

B, HIDDEN = 16, 32
POINTERS = ("x0", "x1", "y", "acts", "dy", "dz", "dx", "grad", "skinny_ws", "masks")
WITH = {"x0": ("x0_dim", "x0_ld"), "x1": ("x1_dim", "x1_ld"), "y": ("y_ld",), "dy": ("dy_ld",), "dx": ("dx_ld",)}
PLAIN = ("acts_ls", "dz_first", "dx_first")

ENV = NS(hazards_locations=[(0.0, 0.0)] * 7, hazard_locations=[(0.0, 0.0)] * 5, dt=0.02, node_normalizer=None)
ARGS = NS(backup_update_interval=20)


class _BarePlan:
    """The registry of update_plan.Plan without an agent behind it."""
    io = update_plan.Plan.io

    def __init__(self):
        self.io_arrays = []


def _agent():
    h = lambda: NS(desc=_lib.Mlp())
    a = NS(device="cpu", hidden=HIDDEN, fold_launches=False, h_l=h(), h_p=h(), h_q1=h(), h_q2=h(), h_extra=[h()])
    a.h_pols = [a.h_p, h()]
    return a


def _build(name):
    """alloc, value_now_io, extra_value_io and plan of one task on a bare workspace / plan, the way Plan.__init__ and
    _Workspace.__init__ drive them."""
    a = _agent()
    task = tasks.TASKS[name](a, ENV, ARGS)
    lay = a.lay = update_plan._Layout(task)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    NP = task.n_pol
    ws = NS(B=B, nblk=(B + 255) // 256, mb=z(B, lay.LD), pi2=z(NP * B, lay.act_dim), qpi=z(2, NP * B))
    task.alloc(ws)
    P = _BarePlan()
    P.NP = NP
    P.n_q5_count = 2 * NP + 1 + len(task.extra_value_nets())
    io = P.io_q5 = P.io(P.n_q5_count)
    for i in range(2 * NP):          # Q1, Q2 of each controller on (obs, its action)
        io[i].x0, io[i].x0_dim, io[i].x0_ld = ws.mb.data_ptr(), lay.obs_dim, lay.LD
        io[i].x1, io[i].x1_dim, io[i].x1_ld = ws.pi2[i // 2 * B:].data_ptr(), lay.act_dim, lay.act_dim
        io[i].y, io[i].y_ld = ws.qpi[i % 2, i // 2 * B:].data_ptr(), 1
    task.value_now_io(ws, io, 2 * NP)
    task.extra_value_io(ws, io, 2 * NP + 1)
    task.plan(ws, P)
    return task, ws, P


def _resolver(ws):
    """address -> "buffer+byte offset": the first workspace attribute (in the order they were made) whose storage holds it"""
    spans = []
    for name, t in vars(ws).items():
        if isinstance(t, torch.Tensor):
            st = t.untyped_storage()
            if all(st.data_ptr() != s[0] for s in spans):
                spans.append((st.data_ptr(), st.nbytes(), name))

    def where(p):
        for base, n, name in spans:
            if base <= p < base + n:
                return "%s+%d" % (name, p - base)
        raise AssertionError("pointer %#x is in no workspace buffer" % p)
    return where


def _entry(e, where):
    out = []
    for f in POINTERS:
        p = getattr(e, f)
        if p:
            out.append("%s=%s" % (f, where(p)) + "".join("/%d" % getattr(e, g) for g in WITH.get(f, ())))
        else:
            assert all(getattr(e, g) == 0 for g in WITH.get(f, ())), f
    out += ["%s=%d" % (f, getattr(e, f)) for f in PLAIN if getattr(e, f)]
    return " ".join(out)


def _io_rows(name):
    """per registered array, in registration order: its entries as strings"""
    _, ws, P = _build(name)
    where = _resolver(ws)
    return [[_entry(e, where) for e in arr] for arr in P.io_arrays]


def _facts(name):
    t = _build(name)[0]
    return dict(n_pol=t.n_pol, n_eps=t.n_eps, eps_order=t.eps_order, backup_mode=t.backup_mode, ratio_mode=t.ratio_mode,
                lam_hi=t.lam_hi, rollout_waits=t.rollout_waits, graph_ok=t.graph_ok, has_signal=t.has_signal,
                n_extra_critics=t.n_extra_critics, num_cbfs=t.num_cbfs, gamma_l=t.gamma_l,
                backup_interval=t.backup_interval, n_pol_now=(t.n_pol_now(0), t.n_pol_now(20)),
                backup_lam_due=t.backup_lam_due(40, 2), fit_due=t.fit_due(101),
                lya_train_cols=t.lya_train_cols(NS(lya="lya", nlya="nlya", obs="obs", nobs="nobs")),
                fit_ws={k: tuple(v.shape) for k, v in t.fit_ws(32).items()})


def _fit_ws(n_s):
    return dict(st=(32, n_s), nst=(32, n_s), dpred=(32, n_s), part=(1,), u=(32, 2))


# the learned-barrier pattern: one controller, no backup, barrier signal in the replay rows, BarrierNet beside the critics
_BARRIER = dict(n_pol=1, n_eps=3, eps_order=None, backup_mode=0, rollout_waits=1, has_signal=True, n_extra_critics=1,
                num_cbfs=1, backup_interval=1, n_pol_now=(1, 1), backup_lam_due=0, lam_hi=400.0)

FACTS = {
    "Unicycle": dict(n_pol=2, n_eps=3, eps_order=None, backup_mode=1, ratio_mode=1, lam_hi=400.0, rollout_waits=1,
                     graph_ok=True, has_signal=False, n_extra_critics=0, num_cbfs=7, gamma_l=1.0, backup_interval=1,
                     n_pol_now=(2, 2), backup_lam_due=1, fit_due=True, lya_train_cols=("lya", "nlya"),
                     fit_ws=_fit_ws(3)),
    "SimulatedCars": dict(n_pol=2, n_eps=5, eps_order=None, backup_mode=1, ratio_mode=2, lam_hi=300.0, rollout_waits=2,
                          graph_ok=False, has_signal=False, n_extra_critics=0, num_cbfs=2, gamma_l=0.15,
                          backup_interval=1, n_pol_now=(2, 2), backup_lam_due=1, fit_due=True,
                          lya_train_cols=("lya", "nlya"), fit_ws=_fit_ws(10)),
    "Pvtol": dict(n_pol=2, n_eps=7, eps_order=[0, 1, 4, 2, 5, 3, 6], backup_mode=2, ratio_mode=2, lam_hi=400.0,
                  rollout_waits=3, graph_ok=False, has_signal=False, n_extra_critics=0, num_cbfs=9, gamma_l=0.1,
                  backup_interval=20, n_pol_now=(2, 2), backup_lam_due=1, fit_due=False,
                  lya_train_cols=("obs", "nobs"), fit_ws=_fit_ws(6)),
    # (its backup-multiplier flag still follows the shared schedule; with backup_mode 0 no kernel reads it)
    "UnicycleBarrier": dict(_BARRIER, backup_lam_due=1, ratio_mode=0, graph_ok=True, gamma_l=1.0, fit_due=True,
                            lya_train_cols=("lya", "nlya"), fit_ws=_fit_ws(3)),
    "PvtolBarrier": dict(_BARRIER, ratio_mode=2, graph_ok=False, gamma_l=0.1, fit_due=False,
                         lya_train_cols=("obs", "nobs"), fit_ws=_fit_ws(6)),
    # fits the NODE only in episodes <= 100 and regresses the Lyapunov critic on observations, as PvtolBarrier does
    "QuadrotorBarrier": dict(_BARRIER, ratio_mode=2, graph_ok=False, gamma_l=0.1, fit_due=False,
                             lya_train_cols=("obs", "nobs"), fit_ws=_fit_ws(6)),
}

# task -> the arrays of Plan.io_arrays in registration order, each a list of its entries:
# field=buffer+byte offset[/dim]/ld of every non-null pointer, then the non-zero plain fields
IO = {
    "Unicycle": [
        ["x0=mb+0/7/28 x1=pi2+0/2/2 y=qpi+0/1",
         "x0=mb+0/7/28 x1=pi2+0/2/2 y=qpi+128/1",
         "x0=mb+0/7/28 x1=pi2+128/2/2 y=qpi+64/1",
         "x0=mb+0/7/28 x1=pi2+128/2/2 y=qpi+192/1",
         "x0=mb+44/2/28 y=V+0/1"],
        ["x0=ps_next2+0/2/2 y=Vn+0/1 acts=acts_vn+0 dy=dVn+0/1 dx=dps_v2+0/2"],
        ["x0=mb+0/7/28 x1=pi2+0/2/2 y=qpi+0/1",
         "x0=mb+0/7/28 x1=pi2+0/2/2 y=qpi+128/1",
         "x0=mb+0/7/28 x1=pi2+128/2/2 y=qpi+64/1",
         "x0=mb+0/7/28 x1=pi2+128/2/2 y=qpi+192/1",
         "x0=ps_next2+0/2/2 y=Vn+0/1 acts=acts_vn+0 dy=dVn+0/1 dx=dps_v2+0/2"],
        ["x0=mb+0/7/28 x1=pi2+0/2/2 y=qpi+0/1",
         "x0=mb+0/7/28 x1=pi2+0/2/2 y=qpi+128/1",
         "x0=mb+0/7/28 x1=pi2+128/2/2 y=qpi+64/1",
         "x0=mb+0/7/28 x1=pi2+128/2/2 y=qpi+192/1",
         "x0=mb+44/2/28 y=V+0/1",
         "x0=ps_next2+0/2/2 y=Vn+0/1 acts=acts_vn+0 dy=dVn+0/1 dx=dps_v2+0/2"],
    ],
    "SimulatedCars": [
        ["x0=mb+0/10/36 x1=pi2+0/1/1 y=qpi+0/1",
         "x0=mb+0/10/36 x1=pi2+0/1/1 y=qpi+128/1",
         "x0=mb+0/10/36 x1=pi2+64/1/1 y=qpi+64/1",
         "x0=mb+0/10/36 x1=pi2+64/1/1 y=qpi+192/1",
         "x0=mb+52/4/36 y=V+0/1"],
        ["x0=x1_2+16/4/10 y=V1+0/1 acts=acts_v1+0 dy=dV1+0/1 dx=dlya+0/4"],
        ["x0=obs1_2+0/10/10 y=heads_nx+0/2",
         "x0=obs1_2+640/10/10 y=heads_nx+128/2"],
    ],
    "UnicycleBarrier": [
        ["x0=mb+0/7/28 x1=pi2+0/2/2 y=qpi+0/1",
         "x0=mb+0/7/28 x1=pi2+0/2/2 y=qpi+64/1",
         "x0=mb+48/2/28 y=V+0/1",
         "x0=mb+0/7/28 x1=pi2+0/2/2 y=Bv+0/1"],
        ["x0=lya_next+0/2/2 y=Vn+0/1 acts=acts_vn+0 dy=dVn+0/1 dx=dlya_next+0/2"],
        ["x0=obs_pred+0/7/7 y=heads_nx+0/4"],
        ["x0=obs_pred+0/7/7 x1=pi_next+0/2/2 y=Bn+0/1 acts=acts_bn+0 dy=dBn+0/1 dx=dxb+0/9"],
    ],
    "Pvtol": [
        ["x0=mb+0/11/52 x1=pi2+0/2/2 y=qpi+0/1",
         "x0=mb+0/11/52 x1=pi2+0/2/2 y=qpi+128/1",
         "x0=mb+0/11/52 x1=pi2+128/2/2 y=qpi+64/1",
         "x0=mb+0/11/52 x1=pi2+128/2/2 y=qpi+192/1",
         "x0=mb+60/11/52 y=V+0/1"],
        ["x0=obs1+0/11/11 y=V1+0/1 acts=acts_v1+0 dy=dV1+0/1 dx=dobs1+0/11"],
        ["x0=obs1+0/11/11 y=heads_n1+0/4",
         "x0=obs1+704/11/11 y=heads_n1+256/4"],
        ["x0=obs2+0/11/11 y=heads_n2+0/4",
         "x0=obs2+704/11/11 y=heads_n2+256/4"],
    ],
    "PvtolBarrier": [
        ["x0=mb+0/11/52 x1=pi2+0/2/2 y=qpi+0/1",
         "x0=mb+0/11/52 x1=pi2+0/2/2 y=qpi+64/1",
         "x0=mb+64/11/52 y=V+0/1",
         "x0=mb+0/11/52 x1=pi2+0/2/2 y=Bv+0/1"],
        ["x0=obs_pred+0/11/11 y=Vn+0/1 acts=acts_vn+0 dy=dVn+0/1 dx=dlya_next+0/11"],
        ["x0=obs_pred+0/11/11 y=heads_nx+0/4"],
        ["x0=obs_pred+0/11/11 x1=pi_next+0/2/2 y=Bn+0/1 acts=acts_bn+0 dy=dBn+0/1 dx=dxb+0/13"],
    ],
    "QuadrotorBarrier": [
        ["x0=mb+0/6/32 x1=pi2+0/2/2 y=qpi+0/1",
         "x0=mb+0/6/32 x1=pi2+0/2/2 y=qpi+64/1",
         "x0=mb+44/6/32 y=V+0/1",
         "x0=mb+0/6/32 x1=pi2+0/2/2 y=Bv+0/1"],
        ["x0=obs_pred+0/6/6 y=Vn+0/1 acts=acts_vn+0 dy=dVn+0/1 dx=dx_next+0/6"],
        ["x0=obs_pred+0/6/6 y=heads_nx+0/4"],
        ["x0=obs_pred+0/6/6 x1=pi_next+0/2/2 y=Bn+0/1 acts=acts_bn+0 dy=dBn+0/1 dx=dxb+0/8"],
    ],
}


@pytest.fixture(autouse=True)
def _no_launches(monkeypatch):
    def boom(name, *args):
        raise AssertionError("%s launched from a host-only test" % name)
    monkeypatch.setattr(_lib, "call", boom)


def test_every_task_is_covered():
    assert set(tasks.TASKS) == set(FACTS) == set(IO) and len(tasks.TASKS) == 6


@pytest.mark.parametrize("name", sorted(FACTS))
def test_class_level_facts(name):
    got = _facts(name)
    assert got == FACTS[name], {k: (got[k], FACTS[name][k]) for k in got if got[k] != FACTS[name][k]}
    assert tasks.TASKS[name].name == name
    # Pvtol alone alternates: the backup controller joins every 20th update, its multiplier every 20th interval
    if name == "Pvtol":
        t = _build(name)[0]
        assert [t.n_pol_now(u) for u in (0, 1, 19, 20, 21)] == [2, 1, 1, 2, 1]
        assert [t.backup_lam_due(u, 2) for u in (0, 2, 20, 40, 80)] == [1, 0, 0, 1, 1]
        assert t.fit_due(None) and t.fit_due(100)


@pytest.mark.parametrize("name", sorted(FACTS))
def test_launch_descriptors(name):
    got = _io_rows(name)
    assert [len(a) for a in got] == [len(a) for a in IO[name]]
    for k, (g, w) in enumerate(zip(got, IO[name])):
        assert g == w, "array %d of %s" % (k, name)
