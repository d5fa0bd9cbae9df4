"""CPU: every head structure a plan builds (``update_plan.Plan.heads`` and the tasks' ``plan``) for the six tasks with
the launch folds on, rendered field by field with every pointer resolved to the buffer (name + byte offset) it lands
in, against literal tables.  No kernel is launched: the plan is built over a stand-in agent whose nets and arenas are
laid out on the host the way ``SAC_CBF_CLF.__init__`` lays them out on the device.

Where the tables come from: they were not written from the code under test.  ``dump`` below was run on an MI355X over
real agents (B = 16, hidden 256) after their first update with both controllers (update 0; update 20 for Pvtol's
NP = 2), once at the commit before the heads moved into the plan — which built them inside the launch functions on
first use — and once on this tree; the two dumps were identical text, per-update fields included.  ``HEADS`` is that
dump without the fields ``PER_UPDATE`` names, which the launch sites store on every update."""
import ctypes as C
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn as nn

import nlbac_amd  # noqa: F401
from nlbac_amd import _lib, synth
from nlbac_amd.arena import Arena
from nlbac_amd.sac_cbf_clf import _layout as SC
from nlbac_amd.sac_cbf_clf import model, tasks, update_plan

B, HIDDEN = 16, 256
# what a launch site stores per update: excluded from the tables wherever it occurs in a path
PER_UPDATE = ("do_lambda_update", "do_backup_lambda_update", "cf_do_lambda_update", "cf_do_backup_lambda_update",
              "cb_defer", "cb_partials", "cb_tiles", "cb_stage", "cb_auglag", "finish[2]", "da[2]", "da_ld[2]")
CASES = {"Unicycle": ("Unicycle", 2), "SimulatedCars": ("SimulatedCars", 2), "Pvtol/1": ("Pvtol", 1), "Pvtol/2": ("Pvtol", 2),
         "UnicycleBarrier": ("UnicycleBarrier", 1), "PvtolBarrier": ("PvtolBarrier", 1),
         "QuadrotorBarrier": ("QuadrotorBarrier", 1)}


def plan_heads(P):
    """name -> head structure (or None) of a plan, the task's own included"""
    out = {n: getattr(P, n) for n in ("auglag", "head_pol3", "head_td", "actor_scalars", "head_actor_q", "head_gauss")}
    out.update({n: getattr(P, n) for n in ("cf_head", "head_actor_q_cb") if hasattr(P, n)})
    nx = getattr(P, "head_nx", None)
    out.update({"head_nx[%d]" % i: h for i, h in enumerate(nx)} if isinstance(nx, list) else {"head_nx": nx})
    return out


def resolver(agent, ws):
    """address -> "owner.buffer+byte offset" over everything a head may point into; anything else fails"""
    named = [("ws." + k, t) for k, t in vars(ws).items() if isinstance(t, torch.Tensor)]
    named += [("sc", agent.sc), ("tickets", agent._tickets), ("policy.action_scale", agent.policy.action_scale),
              ("policy.action_bias", agent.policy.action_bias)]
    for k in ("ar_c", "ar_a", "ar_b"):
        if getattr(agent, k, None) is not None:
            named += [(k + ".theta", getattr(agent, k).theta), (k + ".grad", getattr(agent, k).grad)]
    if hasattr(agent.task, "hazards"):
        named.append(("task.hazards", agent.task.hazards))
    spans = []
    for name, t in named:          # (views share storage: the first name made for a storage stands for it)
        st = t.untyped_storage()
        if all(st.data_ptr() != s[0] for s in spans):
            spans.append((st.data_ptr(), st.nbytes(), name))

    def where(p):
        for base, n, name in spans:
            if base <= p < base + n:
                return "%s+%d" % (name, p - base)
        raise AssertionError("pointer %#x lands in none of the owners" % p)
    return where


def dump(x, typ, path, where, skip=()):
    """One ``path=value`` per non-null pointer / non-zero scalar below ``x``, through nested structures and arrays."""
    if set(path.split(".")) & set(skip):
        return []
    if issubclass(typ, C.Structure):
        return [l for f, t in typ._fields_ for l in dump(getattr(x, f), t, (path + "." if path else "") + f, where, skip)]
    if issubclass(typ, C.Array):
        return [l for i in range(typ._length_) for l in dump(x[i], typ._type_, "%s[%d]" % (path, i), where, skip)]
    if not x:
        return []
    if typ is C.c_void_p:
        return ["%s=%s" % (path, where(x))]
    return ["%s=%s" % (path, "%.9g" % x if typ in (C.c_float, C.c_double) else "%d" % x)]


def render(heads, where, skip=()):
    """name -> one string of all its fields (None: the head does not exist)"""
    return {n: None if h is None else " ".join(dump(h, type(h), "", where, skip)) for n, h in heads.items()}


def stand_in_agent(name, fold=True, defer=True):
    """What ``Plan`` reads of an agent, with the nets, arenas and log alphas laid out as SAC_CBF_CLF.__init__ does."""
    from oracle.nlbac_oracle import Args
    env, dev = synth.fixture_env({"QuadrotorBarrier": "QuadrotorLike"}.get(name, name), 0), torch.device("cpu")
    args = Args(batch_size=B, hidden_size=HIDDEN, seed=0, cuda=True)
    a = NS(device=dev, hidden=HIDDEN, env=env, fold_launches=fold, sums_defer=defer, world=1, gamma=args.gamma,
           gamma_b=args.gamma_b, batch_size=args.batch_size, solver="euler", atol=1e-7, rtol=1e-5)
    task = a.task = tasks.TASKS[name](a, env, args)
    a.lay = update_plan._Layout(task)
    Do, Da, n_pol = task.obs_dim, task.act_dim, task.n_pol
    a.target_entropy = -float(Da)
    log_alpha, backup_log_alpha = nn.Parameter(torch.zeros(1)), nn.Parameter(torch.zeros(1))
    a.policy = model.GaussianPolicy(Do, Da, HIDDEN, env.action_space)
    backup = model.GaussianPolicy(Do, Da, HIDDEN, env.action_space) if n_pol == 2 else None
    a.neural_ode_model = task.build_node()
    a.ar_c, a.ar_a, a.ar_n = Arena(dev, 8, with_target=True), Arena(dev, 8), Arena(dev, 2)
    a.h_q1, a.h_q2 = model.QNetwork(Do, Da, HIDDEN).attach(a.ar_c)
    (a.h_l,) = model.LyaNetwork(task.lya_dim, HIDDEN).attach(a.ar_c)
    a.h_extra = list(model.BarrierNetwork(Do, Da, HIDDEN).attach(a.ar_c)) if task.has_signal else []
    (a.h_p,) = a.policy.attach(a.ar_a)
    a.h_pols = [a.h_p]
    a.ar_b = Arena(dev, 8) if (n_pol == 2 and task.backup_interval > 1) else None
    ar_backup = a.ar_b if a.ar_b is not None else a.ar_a
    if n_pol == 2:
        a.h_pols.append(backup.attach(ar_backup)[0])
    a.ar_a.add_group([log_alpha])
    if n_pol == 2:
        ar_backup.add_group([backup_log_alpha])
    h_node = list(a.neural_ode_model.attach(a.ar_n))
    for ar in (a.ar_c, a.ar_a, a.ar_b, a.ar_n):
        if ar is not None:
            ar.finalize()
    a.h_crit = [a.h_q1, a.h_q2, a.h_l] + a.h_extra
    for h in a.h_crit + a.h_pols + h_node:
        h.bind()
    la_off = a.ar_a.offset_of[id(log_alpha)]
    if a.ar_b is not None:
        a.actor_groups = [NS(arena=a.ar_a, first=0, count=1, la_off=la_off, la_stride=0),
                          NS(arena=a.ar_b, first=1, count=1, la_stride=0, la_off=a.ar_b.offset_of[id(backup_log_alpha)])]
    else:
        stride = (a.ar_a.offset_of[id(backup_log_alpha)] - la_off) if n_pol == 2 else 0
        a.actor_groups = [NS(arena=a.ar_a, first=0, count=n_pol, la_off=la_off, la_stride=stride)]
    a.pol_arena = [a.ar_a] + ([ar_backup] if n_pol == 2 else [])
    a.sc = torch.zeros(SC.SC_SIZE, dtype=torch.float32)
    a._tickets = torch.zeros(16, dtype=torch.int32)
    task.setup()
    return a


def build(case, fold=True, defer=True):
    name, NP = CASES[case]
    a = stand_in_agent(name, fold, defer)
    ws = update_plan._Workspace(B, HIDDEN, a.device, a.lay, a.task)
    return a, ws, update_plan.Plan(a, ws, NP)


def rendered(case, fold=True, defer=True):
    a, ws, P = build(case, fold, defer)
    return render(plan_heads(P), resolver(a, ws), PER_UPDATE)


# case -> head -> its non-null pointers (buffer+byte offset) and non-zero scalars, PER_UPDATE fields left out
HEADS = {
    "Unicycle": {
        "auglag": "n_cbf=7 n_clf=1 batch_size=16 ratio_mode=1 backup_mode=1 lam_lo=0.00999999978 lam_hi=400",
        "head_pol3": (
            "eps=ws.eps+0 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.act3+0 "
            "action_ld=2 logp=ws.logp3+0"),
        "head_td": (
            "kind=2 B_norm=16 alpha=sc+0 q1t=ws.q6+0 q2t=ws.q6+64 lt=ws.q6+128 nlogp=ws.logp3+0 reward=ws.mb+36 "
            "constraint=ws.mb+40 mask=ws.mb+88 rcm_ld=28 q[0]=ws.q6+192 q[1]=ws.q6+256 q[2]=ws.q6+320 "
            "gamma=0.99000001 dq[0]=ws.dq3+0 dq[1]=ws.dq3+64 dq[2]=ws.dq3+128 next_q=ws.next_q+0 "
            "next_l=ws.next_l+0 partials=ws.part_td32+0 ticket=ws.tickets_td+0 mul=0.0625 out=sc+28 sums_defer=1 "
            "sums_tiles=ws.sums_tiles+0"),
        "actor_scalars": None,
        "head_actor_q": (
            "kind=3 B_norm=16 alpha=sc+0 qa=ws.qpi+0 qb=ws.qpi+128 logp=ws.logp3+64 dqa=ws.dq_pi+0 "
            "dqb=ws.dq_pi+128 n_prob=2 actor.target_entropy=-2 actor.log_alpha[0]=ar_a.theta+550944 "
            "actor.log_alpha[1]=ar_a.theta+550960 actor.g_log_alpha[0]=ar_a.grad+550944 "
            "actor.g_log_alpha[1]=ar_a.grad+550960 actor.sc=sc+0 partials=ws.part_q32+0 ticket=ws.tickets_q+0 "
            "sums_defer=1 sums_tiles=ws.sums_tiles+4"),
        "head_gauss": (
            "kind=1 B_norm=16 heads=ws.heads3+256 heads_ld=4 eps=ws.eps+128 scale=policy.action_scale+0 n_u=2 "
            "da[0]=ws.dxq+28 da[1]=ws.dxq+1180 da_ld[0]=9 da_ld[1]=9 alpha=sc+0 dlogp_mul=0.0625 "
            "dheads=ws.dheads2+0 dheads_ld=4 finish[0].kind=2 finish[0].n_nets=3 "
            "finish[0].partials=ws.part_td32+0 finish[0].n_tiles=ws.sums_tiles+0 finish[0].mul=0.0625 "
            "finish[0].out=sc+28 finish[1].kind=3 finish[1].n_nets=2 finish[1].partials=ws.part_q32+0 "
            "finish[1].n_tiles=ws.sums_tiles+4 finish[1].B_norm=16 finish[1].actor.target_entropy=-2 "
            "finish[1].actor.log_alpha[0]=ar_a.theta+550944 finish[1].actor.log_alpha[1]=ar_a.theta+550960 "
            "finish[1].actor.g_log_alpha[0]=ar_a.grad+550944 finish[1].actor.g_log_alpha[1]=ar_a.grad+550960 "
            "finish[1].actor.sc=sc+0"),
        "cf_head": (
            "cf_kind=1 cf_nh=7 cf_ps=ws.ps+0 cf_ps_next=ws.ps_next2+0 cf_V=ws.V+0 cf_hazards=task.hazards+0 "
            "cf_r2=0.275624961 cf_dt=0.0199999996 cf_gamma_b=50 cf_gamma_l=1 cf_matr=ws.matr+0 "
            "cf_bmatr=ws.bmatr+0 cf_partials=ws.part_c16+0 cf_tickets=ws.tickets_c+0 cf_n_cbf=7 cf_n_clf=1 "
            "cf_batch_size=16 cf_ratio_mode=1 cf_backup_mode=1 cf_lam_lo=0.00999999978 cf_lam_hi=400 cf_sc=sc+0 "
            "cf_defer=1 cf_tiles=ws.sums_tiles+8"),
        "head_actor_q_cb": (
            "kind=3 B_norm=16 alpha=sc+0 qa=ws.qpi+0 qb=ws.qpi+128 logp=ws.logp3+64 dqa=ws.dq_pi+0 "
            "dqb=ws.dq_pi+128 n_prob=2 actor.target_entropy=-2 actor.log_alpha[0]=ar_a.theta+550944 "
            "actor.log_alpha[1]=ar_a.theta+550960 actor.g_log_alpha[0]=ar_a.grad+550944 "
            "actor.g_log_alpha[1]=ar_a.grad+550960 actor.sc=sc+0 partials=ws.part_q32+0 ticket=ws.tickets_q+0 "
            "cb_kind=1 cb_nh=7 cb_ps_next=ws.ps_next2+0 cb_matr=ws.matr+0 cb_bmatr=ws.bmatr+0 "
            "cb_hazards=task.hazards+0 cb_sc=sc+0 cb_dt=0.0199999996 cb_batch=16 cb_dps_next=ws.dps_next2+0 "
            "cb_dV=ws.dVn+0 sums_defer=1 sums_tiles=ws.sums_tiles+4"),
        "head_nx": None,
    },
    "SimulatedCars": {
        "auglag": "n_cbf=2 n_clf=1 batch_size=16 ratio_mode=2 backup_mode=1 lam_lo=0.00999999978 lam_hi=300",
        "head_pol3": (
            "eps=ws.eps+0 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=1 action=ws.act3+0 "
            "action_ld=1 logp=ws.logp3+0"),
        "head_td": (
            "kind=2 B_norm=16 alpha=sc+0 q1t=ws.q6+0 q2t=ws.q6+64 lt=ws.q6+128 nlogp=ws.logp3+0 reward=ws.mb+44 "
            "constraint=ws.mb+48 mask=ws.mb+124 rcm_ld=36 q[0]=ws.q6+192 q[1]=ws.q6+256 q[2]=ws.q6+320 "
            "gamma=0.99000001 dq[0]=ws.dq3+0 dq[1]=ws.dq3+64 dq[2]=ws.dq3+128 next_q=ws.next_q+0 "
            "next_l=ws.next_l+0 partials=ws.part_td32+0 ticket=ws.tickets_td+0 mul=0.0625 out=sc+28 sums_defer=1 "
            "sums_tiles=ws.sums_tiles+0"),
        "actor_scalars": None,
        "head_actor_q": (
            "kind=3 B_norm=16 alpha=sc+0 qa=ws.qpi+0 qb=ws.qpi+128 logp=ws.logp3+64 dqa=ws.dq_pi+0 "
            "dqb=ws.dq_pi+128 n_prob=2 actor.target_entropy=-1 actor.log_alpha[0]=ar_a.theta+552992 "
            "actor.log_alpha[1]=ar_a.theta+553008 actor.g_log_alpha[0]=ar_a.grad+552992 "
            "actor.g_log_alpha[1]=ar_a.grad+553008 actor.sc=sc+0 partials=ws.part_q32+0 ticket=ws.tickets_q+0 "
            "sums_defer=1 sums_tiles=ws.sums_tiles+4"),
        "head_gauss": (
            "kind=1 B_norm=16 heads=ws.heads3+128 heads_ld=2 eps=ws.eps+64 scale=policy.action_scale+0 n_u=1 "
            "da[0]=ws.dxq+40 da[1]=ws.dxq+1448 da_ld[0]=11 da_ld[1]=11 alpha=sc+0 dlogp_mul=0.0625 "
            "dheads=ws.dheads2+0 dheads_ld=2 finish[0].kind=2 finish[0].n_nets=3 "
            "finish[0].partials=ws.part_td32+0 finish[0].n_tiles=ws.sums_tiles+0 finish[0].mul=0.0625 "
            "finish[0].out=sc+28 finish[1].kind=3 finish[1].n_nets=2 finish[1].partials=ws.part_q32+0 "
            "finish[1].n_tiles=ws.sums_tiles+4 finish[1].B_norm=16 finish[1].actor.target_entropy=-1 "
            "finish[1].actor.log_alpha[0]=ar_a.theta+552992 finish[1].actor.log_alpha[1]=ar_a.theta+553008 "
            "finish[1].actor.g_log_alpha[0]=ar_a.grad+552992 finish[1].actor.g_log_alpha[1]=ar_a.grad+553008 "
            "finish[1].actor.sc=sc+0"),
        "head_nx": (
            "eps=ws.eps+192 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=1 action=ws.c2+0 "
            "action_ld=2 logp=ws.logp_nx+0"),
    },
    "Pvtol/1": {
        "auglag": "n_cbf=9 n_clf=1 batch_size=16 ratio_mode=2 lam_lo=0.00999999978 lam_hi=400",
        "head_pol3": (
            "eps=ws.eps+0 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.act3+0 "
            "action_ld=2 logp=ws.logp3+0"),
        "head_td": (
            "kind=2 B_norm=16 alpha=sc+0 q1t=ws.q6+0 q2t=ws.q6+64 lt=ws.q6+128 nlogp=ws.logp3+0 reward=ws.mb+52 "
            "constraint=ws.mb+56 mask=ws.mb+192 rcm_ld=52 q[0]=ws.q6+192 q[1]=ws.q6+256 q[2]=ws.q6+320 "
            "gamma=0.99000001 dq[0]=ws.dq3+0 dq[1]=ws.dq3+64 dq[2]=ws.dq3+128 next_q=ws.next_q+0 "
            "next_l=ws.next_l+0 partials=ws.part_td32+0 ticket=ws.tickets_td+0 mul=0.0625 out=sc+28 sums_defer=1 "
            "sums_tiles=ws.sums_tiles+0"),
        "actor_scalars": None,
        "head_actor_q": (
            "kind=3 B_norm=16 alpha=sc+0 qa=ws.qpi+0 qb=ws.qpi+128 logp=ws.logp3+64 dqa=ws.dq_pi+0 "
            "dqb=ws.dq_pi+128 n_prob=1 actor.target_entropy=-2 actor.log_alpha[0]=ar_a.theta+279568 "
            "actor.g_log_alpha[0]=ar_a.grad+279568 actor.sc=sc+0 partials=ws.part_q32+0 ticket=ws.tickets_q+0 "
            "sums_defer=1 sums_tiles=ws.sums_tiles+4"),
        "head_gauss": (
            "kind=1 B_norm=16 heads=ws.heads3+256 heads_ld=4 eps=ws.eps+128 scale=policy.action_scale+0 n_u=2 "
            "da[0]=ws.dxq+44 da[1]=ws.dxq+1708 da_ld[0]=13 da_ld[1]=13 alpha=sc+0 dlogp_mul=0.0625 "
            "dheads=ws.dheads2+0 dheads_ld=4 finish[0].kind=2 finish[0].n_nets=3 "
            "finish[0].partials=ws.part_td32+0 finish[0].n_tiles=ws.sums_tiles+0 finish[0].mul=0.0625 "
            "finish[0].out=sc+28 finish[1].kind=3 finish[1].n_nets=1 finish[1].partials=ws.part_q32+0 "
            "finish[1].n_tiles=ws.sums_tiles+4 finish[1].B_norm=16 finish[1].actor.target_entropy=-2 "
            "finish[1].actor.log_alpha[0]=ar_a.theta+279568 finish[1].actor.g_log_alpha[0]=ar_a.grad+279568 "
            "finish[1].actor.sc=sc+0"),
        "head_nx[0]": (
            "eps=ws.eps+384 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.a1+0 "
            "action_ld=2 logp=ws.logp_nx+0"),
        "head_nx[1]": (
            "eps=ws.eps+640 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.a2+0 "
            "action_ld=2 logp=ws.logp_nx+0"),
    },
    "Pvtol/2": {
        "auglag": "n_cbf=9 n_clf=1 batch_size=16 ratio_mode=2 backup_mode=2 lam_lo=0.00999999978 lam_hi=400",
        "head_pol3": (
            "eps=ws.eps+0 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.act3+0 "
            "action_ld=2 logp=ws.logp3+0"),
        "head_td": (
            "kind=2 B_norm=16 alpha=sc+0 q1t=ws.q6+0 q2t=ws.q6+64 lt=ws.q6+128 nlogp=ws.logp3+0 reward=ws.mb+52 "
            "constraint=ws.mb+56 mask=ws.mb+192 rcm_ld=52 q[0]=ws.q6+192 q[1]=ws.q6+256 q[2]=ws.q6+320 "
            "gamma=0.99000001 dq[0]=ws.dq3+0 dq[1]=ws.dq3+64 dq[2]=ws.dq3+128 next_q=ws.next_q+0 "
            "next_l=ws.next_l+0 partials=ws.part_td32+0 ticket=ws.tickets_td+0 mul=0.0625 out=sc+28 sums_defer=1 "
            "sums_tiles=ws.sums_tiles+0"),
        "actor_scalars": None,
        "head_actor_q": (
            "kind=3 B_norm=16 alpha=sc+0 qa=ws.qpi+0 qb=ws.qpi+128 logp=ws.logp3+64 dqa=ws.dq_pi+0 "
            "dqb=ws.dq_pi+128 n_prob=2 actor.target_entropy=-2 actor.log_alpha[0]=ar_a.theta+279568 "
            "actor.log_alpha[1]=ar_b.theta+279568 actor.g_log_alpha[0]=ar_a.grad+279568 "
            "actor.g_log_alpha[1]=ar_b.grad+279568 actor.sc=sc+0 partials=ws.part_q32+0 ticket=ws.tickets_q+0 "
            "sums_defer=1 sums_tiles=ws.sums_tiles+4"),
        "head_gauss": (
            "kind=1 B_norm=16 heads=ws.heads3+256 heads_ld=4 eps=ws.eps+128 scale=policy.action_scale+0 n_u=2 "
            "da[0]=ws.dxq+44 da[1]=ws.dxq+1708 da_ld[0]=13 da_ld[1]=13 alpha=sc+0 dlogp_mul=0.0625 "
            "dheads=ws.dheads2+0 dheads_ld=4 finish[0].kind=2 finish[0].n_nets=3 "
            "finish[0].partials=ws.part_td32+0 finish[0].n_tiles=ws.sums_tiles+0 finish[0].mul=0.0625 "
            "finish[0].out=sc+28 finish[1].kind=3 finish[1].n_nets=2 finish[1].partials=ws.part_q32+0 "
            "finish[1].n_tiles=ws.sums_tiles+4 finish[1].B_norm=16 finish[1].actor.target_entropy=-2 "
            "finish[1].actor.log_alpha[0]=ar_a.theta+279568 finish[1].actor.log_alpha[1]=ar_b.theta+279568 "
            "finish[1].actor.g_log_alpha[0]=ar_a.grad+279568 finish[1].actor.g_log_alpha[1]=ar_b.grad+279568 "
            "finish[1].actor.sc=sc+0"),
        "head_nx[0]": (
            "eps=ws.eps+384 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.a1+0 "
            "action_ld=2 logp=ws.logp_nx+0"),
        "head_nx[1]": (
            "eps=ws.eps+640 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.a2+0 "
            "action_ld=2 logp=ws.logp_nx+0"),
    },
    "UnicycleBarrier": {
        "auglag": "n_cbf=1 n_clf=1 batch_size=16 lam_lo=0.00999999978 lam_hi=400",
        "head_pol3": (
            "eps=ws.eps+0 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.act3+0 "
            "action_ld=2 logp=ws.logp3+0"),
        "head_td": (
            "kind=2 B_norm=16 alpha=sc+0 q1t=ws.q6+0 q2t=ws.q6+64 lt=ws.q6+128 nlogp=ws.logp3+0 reward=ws.mb+36 "
            "constraint=ws.mb+40 mask=ws.mb+92 rcm_ld=28 q[0]=ws.q6+192 q[1]=ws.q6+256 q[2]=ws.q6+320 "
            "gamma=0.99000001 dq[0]=ws.dq3+0 dq[1]=ws.dq3+64 dq[2]=ws.dq3+128 next_q=ws.next_q+0 "
            "next_l=ws.next_l+0 xt=ws.q6+384 xsig=ws.mb+44 xsig_ld=28 xq=ws.q6+448 dxq=ws.dq3+192 out_x=sc+60 "
            "partials=ws.part_td32+0 ticket=ws.tickets_td+0 mul=0.0625 out=sc+28 sums_defer=1 "
            "sums_tiles=ws.sums_tiles+0"),
        "actor_scalars": None,
        "head_actor_q": (
            "kind=3 B_norm=16 alpha=sc+0 qa=ws.qpi+0 qb=ws.qpi+64 logp=ws.logp3+64 dqa=ws.dq_pi+0 dqb=ws.dq_pi+64 "
            "n_prob=1 actor.target_entropy=-2 actor.log_alpha[0]=ar_a.theta+275472 "
            "actor.g_log_alpha[0]=ar_a.grad+275472 actor.sc=sc+0 partials=ws.part_q32+0 ticket=ws.tickets_q+0 "
            "sums_defer=1 sums_tiles=ws.sums_tiles+4"),
        "head_gauss": (
            "kind=1 B_norm=16 heads=ws.heads3+256 heads_ld=4 eps=ws.eps+128 scale=policy.action_scale+0 n_u=2 "
            "da[0]=ws.dxq+28 da[1]=ws.dxq+604 da_ld[0]=9 da_ld[1]=9 alpha=sc+0 dlogp_mul=0.0625 "
            "dheads=ws.dheads2+0 dheads_ld=4 finish[0].kind=2 finish[0].n_nets=4 "
            "finish[0].partials=ws.part_td32+0 finish[0].n_tiles=ws.sums_tiles+0 finish[0].mul=0.0625 "
            "finish[0].out=sc+28 finish[0].out_x=sc+60 finish[1].kind=3 finish[1].n_nets=1 "
            "finish[1].partials=ws.part_q32+0 finish[1].n_tiles=ws.sums_tiles+4 finish[1].B_norm=16 "
            "finish[1].actor.target_entropy=-2 finish[1].actor.log_alpha[0]=ar_a.theta+275472 "
            "finish[1].actor.g_log_alpha[0]=ar_a.grad+275472 finish[1].actor.sc=sc+0"),
        "head_nx": (
            "eps=ws.eps+256 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.pi_next+0 "
            "action_ld=2 logp=ws.logp_nx+0"),
    },
    "PvtolBarrier": {
        "auglag": "n_cbf=1 n_clf=1 batch_size=16 ratio_mode=2 lam_lo=0.00999999978 lam_hi=400",
        "head_pol3": (
            "eps=ws.eps+0 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.act3+0 "
            "action_ld=2 logp=ws.logp3+0"),
        "head_td": (
            "kind=2 B_norm=16 alpha=sc+0 q1t=ws.q6+0 q2t=ws.q6+64 lt=ws.q6+128 nlogp=ws.logp3+0 reward=ws.mb+52 "
            "constraint=ws.mb+56 mask=ws.mb+196 rcm_ld=52 q[0]=ws.q6+192 q[1]=ws.q6+256 q[2]=ws.q6+320 "
            "gamma=0.99000001 dq[0]=ws.dq3+0 dq[1]=ws.dq3+64 dq[2]=ws.dq3+128 next_q=ws.next_q+0 "
            "next_l=ws.next_l+0 xt=ws.q6+384 xsig=ws.mb+60 xsig_ld=52 xq=ws.q6+448 dxq=ws.dq3+192 out_x=sc+60 "
            "partials=ws.part_td32+0 ticket=ws.tickets_td+0 mul=0.0625 out=sc+28 sums_defer=1 "
            "sums_tiles=ws.sums_tiles+0"),
        "actor_scalars": None,
        "head_actor_q": (
            "kind=3 B_norm=16 alpha=sc+0 qa=ws.qpi+0 qb=ws.qpi+64 logp=ws.logp3+64 dqa=ws.dq_pi+0 dqb=ws.dq_pi+64 "
            "n_prob=1 actor.target_entropy=-2 actor.log_alpha[0]=ar_a.theta+279568 "
            "actor.g_log_alpha[0]=ar_a.grad+279568 actor.sc=sc+0 partials=ws.part_q32+0 ticket=ws.tickets_q+0 "
            "sums_defer=1 sums_tiles=ws.sums_tiles+4"),
        "head_gauss": (
            "kind=1 B_norm=16 heads=ws.heads3+256 heads_ld=4 eps=ws.eps+128 scale=policy.action_scale+0 n_u=2 "
            "da[0]=ws.dxq+44 da[1]=ws.dxq+876 da_ld[0]=13 da_ld[1]=13 alpha=sc+0 dlogp_mul=0.0625 "
            "dheads=ws.dheads2+0 dheads_ld=4 finish[0].kind=2 finish[0].n_nets=4 "
            "finish[0].partials=ws.part_td32+0 finish[0].n_tiles=ws.sums_tiles+0 finish[0].mul=0.0625 "
            "finish[0].out=sc+28 finish[0].out_x=sc+60 finish[1].kind=3 finish[1].n_nets=1 "
            "finish[1].partials=ws.part_q32+0 finish[1].n_tiles=ws.sums_tiles+4 finish[1].B_norm=16 "
            "finish[1].actor.target_entropy=-2 finish[1].actor.log_alpha[0]=ar_a.theta+279568 "
            "finish[1].actor.g_log_alpha[0]=ar_a.grad+279568 finish[1].actor.sc=sc+0"),
        "head_nx": (
            "eps=ws.eps+256 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.pi_next+0 "
            "action_ld=2 logp=ws.logp_nx+0"),
    },
    "QuadrotorBarrier": {
        "auglag": "n_cbf=1 n_clf=1 batch_size=16 ratio_mode=2 lam_lo=0.00999999978 lam_hi=400",
        "head_pol3": (
            "eps=ws.eps+0 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.act3+0 "
            "action_ld=2 logp=ws.logp3+0"),
        "head_td": (
            "kind=2 B_norm=16 alpha=sc+0 q1t=ws.q6+0 q2t=ws.q6+64 lt=ws.q6+128 nlogp=ws.logp3+0 reward=ws.mb+32 "
            "constraint=ws.mb+36 mask=ws.mb+116 rcm_ld=32 q[0]=ws.q6+192 q[1]=ws.q6+256 q[2]=ws.q6+320 "
            "gamma=0.99000001 dq[0]=ws.dq3+0 dq[1]=ws.dq3+64 dq[2]=ws.dq3+128 next_q=ws.next_q+0 "
            "next_l=ws.next_l+0 xt=ws.q6+384 xsig=ws.mb+40 xsig_ld=32 xq=ws.q6+448 dxq=ws.dq3+192 out_x=sc+60 "
            "partials=ws.part_td32+0 ticket=ws.tickets_td+0 mul=0.0625 out=sc+28 sums_defer=1 "
            "sums_tiles=ws.sums_tiles+0"),
        "actor_scalars": None,
        "head_actor_q": (
            "kind=3 B_norm=16 alpha=sc+0 qa=ws.qpi+0 qb=ws.qpi+64 logp=ws.logp3+64 dqa=ws.dq_pi+0 dqb=ws.dq_pi+64 "
            "n_prob=1 actor.target_entropy=-2 actor.log_alpha[0]=ar_a.theta+274448 "
            "actor.g_log_alpha[0]=ar_a.grad+274448 actor.sc=sc+0 partials=ws.part_q32+0 ticket=ws.tickets_q+0 "
            "sums_defer=1 sums_tiles=ws.sums_tiles+4"),
        "head_gauss": (
            "kind=1 B_norm=16 heads=ws.heads3+256 heads_ld=4 eps=ws.eps+128 scale=policy.action_scale+0 n_u=2 "
            "da[0]=ws.dxq+24 da[1]=ws.dxq+536 da_ld[0]=8 da_ld[1]=8 alpha=sc+0 dlogp_mul=0.0625 "
            "dheads=ws.dheads2+0 dheads_ld=4 finish[0].kind=2 finish[0].n_nets=4 "
            "finish[0].partials=ws.part_td32+0 finish[0].n_tiles=ws.sums_tiles+0 finish[0].mul=0.0625 "
            "finish[0].out=sc+28 finish[0].out_x=sc+60 finish[1].kind=3 finish[1].n_nets=1 "
            "finish[1].partials=ws.part_q32+0 finish[1].n_tiles=ws.sums_tiles+4 finish[1].B_norm=16 "
            "finish[1].actor.target_entropy=-2 finish[1].actor.log_alpha[0]=ar_a.theta+274448 "
            "finish[1].actor.g_log_alpha[0]=ar_a.grad+274448 finish[1].actor.sc=sc+0"),
        "head_nx": (
            "eps=ws.eps+256 scale=policy.action_scale+0 bias=policy.action_bias+0 n_u=2 action=ws.pi_next+0 "
            "action_ld=2 logp=ws.logp_nx+0"),
    },
}


@pytest.fixture(autouse=True)
def _no_launches(monkeypatch):
    def boom(name, *args):
        raise AssertionError("%s launched from a host-only test" % name)
    monkeypatch.setattr(_lib, "call", boom)


def test_every_task_is_covered():
    assert {name for name, _ in CASES.values()} == set(tasks.TASKS) and set(CASES) == set(HEADS)


@pytest.mark.parametrize("case", sorted(CASES))
def test_heads_with_the_folds_on(case):
    got = rendered(case)
    assert set(got) == set(HEADS[case])
    for n in got:
        assert got[n] == HEADS[case][n], "%s of %s" % (n, case)


@pytest.mark.parametrize("case", sorted(CASES))
def test_folds_off_builds_no_head(case):
    """... but the one structure the unfolded update itself passes: nlbac_actor_q_terms' ``actor_scalars``, which in turn
    does not exist with the folds on.  Its fields are the ``actor`` block of the folded update's ``head_actor_q``."""
    a, ws, P = build(case, fold=False)
    off = plan_heads(P)
    assert [n for n, h in off.items() if h is not None] == ["auglag", "actor_scalars"]
    where = resolver(a, ws)
    got = render({"auglag": off["auglag"]}, where, PER_UPDATE)["auglag"]
    assert got == HEADS[case]["auglag"] and HEADS[case]["actor_scalars"] is None
    want = [f.split(".", 1)[1] for f in HEADS[case]["head_actor_q"].split() if f.startswith("actor.")]
    assert dump(off["actor_scalars"], _lib.ActorScalarArgs, "", where) == want and len(want) >= 4


@pytest.mark.parametrize("case", sorted(CASES))
def test_sums_defer_off_removes_exactly_the_deferral(case):
    on, off = rendered(case), rendered(case, defer=False)
    gone = ("sums_defer", "sums_tiles", "cf_defer", "cf_tiles", "finish[0]", "finish[1]")
    for n, text in on.items():
        if text is None:
            assert off[n] is None
            continue
        kept = [f for f in text.split() if not f.startswith(gone)]
        assert off[n].split() == kept, n
    dropped = {f.split("=")[0].split(".")[0] for n, text in on.items() if text for f in text.split() if f.startswith(gone)}
    assert {"sums_defer", "sums_tiles", "finish[0]", "finish[1]"} <= dropped
    assert ("cf_defer" in dropped) == ("cf_tiles" in dropped) == (case == "Unicycle")
