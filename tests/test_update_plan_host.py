"""CPU: the pass that trades saved activation rows for ReLU mask words works on every launch descriptor a plan has
registered, wherever the plan keeps the array; the agent's host modules declare their state (no ``__dict__`` probing).
No kernel is launched here."""
import ctypes as C
import os

import nlbac_amd  # noqa: F401
from nlbac_amd.sac_cbf_clf import update_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Buf:
    """A host stand-in for a device tensor: some bytes with an address."""

    def __init__(self, n=64):
        self.mem = (C.c_char * n)()

    def data_ptr(self):
        return C.addressof(self.mem)


class _BarePlan:
    """The registry of update_plan.Plan without an agent behind it."""
    io = update_plan.Plan.io

    def __init__(self):
        self.io_arrays = []


def test_mask_pass_sees_every_registered_array_and_drops_only_unpaired_activation_rows():
    P = _BarePlan()
    a_trained, a_dx_only, a_shared, dz = _Buf(), _Buf(), _Buf(), _Buf()
    fwd = P.io(2)                               # a forward launch: one trained net, one that is differentiated w.r.t. x only
    fwd[0].acts, fwd[1].acts = a_trained.data_ptr(), a_dx_only.data_ptr()
    bwd = P.io(1)                               # the trained net's backward: the ONLY descriptor that pairs its rows with dz
    bwd[0].acts, bwd[0].dz = a_trained.data_ptr(), dz.data_ptr()
    in_list = [P.io(1), P.io(2)]                # arrays the plan keeps in a container, as a task's per-step lists are
    in_list[0][0].acts = a_dx_only.data_ptr()
    in_list[1][0].acts, in_list[1][1].acts = a_shared.data_ptr(), a_shared.data_ptr()
    no_acts = P.io(1)                           # a value-only launch saves nothing and gets nothing
    assert len(P.io_arrays) == 5 and all(a is b for a, b in zip(P.io_arrays, [fwd, bwd] + in_list + [no_acts]))

    bufs, made = {}, []

    def alloc():
        made.append(_Buf())
        return made[-1]
    update_plan.keep_masks_drop_unpaired_acts(P.io_arrays, bufs, alloc)

    # paired with dz in any one descriptor: the rows stay in all descriptors, and the mask words come too
    assert fwd[0].acts == bwd[0].acts == a_trained.data_ptr()
    assert fwd[0].masks == bwd[0].masks == bufs[a_trained.data_ptr()].data_ptr() != 0
    # never paired: rows dropped, mask words kept — also in the array that was registered from inside a list
    assert fwd[1].acts is None and in_list[0][0].acts is None
    assert fwd[1].masks == in_list[0][0].masks == bufs[a_dx_only.data_ptr()].data_ptr() != 0
    # two descriptors sharing an activation buffer share its mask buffer
    assert in_list[1][0].acts is None and in_list[1][1].acts is None
    assert in_list[1][0].masks == in_list[1][1].masks == bufs[a_shared.data_ptr()].data_ptr() != 0
    assert not no_acts[0].acts and not no_acts[0].masks
    assert len(made) == len(bufs) == 3 and len({b.data_ptr() for b in made}) == 3
    # a second plan of the same workspace (same ``bufs``) reuses the buffers, and decides by its OWN descriptors
    P2 = _BarePlan()
    again = P2.io(1)
    again[0].acts = a_trained.data_ptr()
    update_plan.keep_masks_drop_unpaired_acts(P2.io_arrays, bufs, alloc)
    assert len(made) == 3 and again[0].acts is None and again[0].masks == fwd[0].masks


def test_gradient_and_skinny_partial_consumers_keep_the_rows_too():
    for field in ("grad", "skinny_ws"):
        P = _BarePlan()
        acts, other = _Buf(), _Buf()
        fwd, bwd_w = P.io(1), P.io(1)
        fwd[0].acts = bwd_w[0].acts = acts.data_ptr()
        setattr(bwd_w[0], field, other.data_ptr())
        update_plan.keep_masks_drop_unpaired_acts(P.io_arrays, {}, _Buf)
        assert fwd[0].acts == bwd_w[0].acts == acts.data_ptr() and fwd[0].masks == bwd_w[0].masks != 0


def test_agent_host_modules_declare_their_state():
    pkg = os.path.dirname(update_plan.__file__)
    for name in ("sac_cbf_clf.py", "tasks.py", "update_plan.py", "scalars_readback.py"):
        assert "__dict__" not in open(os.path.join(pkg, name)).read(), name
