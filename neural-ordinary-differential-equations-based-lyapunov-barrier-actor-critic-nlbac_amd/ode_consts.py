"""Constants of the NODE solvers (``odeint.py``): the Butcher tableaus, the fields of the dopri5 control block and the
environment switches."""
import os

# The fields of a problem's dopri5 control block (_lib.DOPRI_CTL doubles): the host's names of the ``C_*`` enumerators of
# csrc/ode_control.h, the one definition on this side (tests/test_abi_and_host.py holds the two together).  Plain ints:
# the accept decision is read on the host's critical path.  Slot 14 is unused; CTL_SEQ exists in the host's copy only.
CTL_H, CTL_T, CTL_RATIO, CTL_ACCEPT, CTL_DONE, CTL_X = 0, 1, 2, 3, 4, 5
CTL_H0, CTL_D0, CTL_D1, CTL_D2 = 6, 7, 8, 9
CTL_NSTEPS, CTL_HUSED, CTL_NACC, CTL_OVF = 10, 11, 12, 13
CTL_SEQ = 15


def ctl_field_ptr(base_ptr, field):
    """Device address of ``field`` (a ``CTL_*``) of the first problem's control block at ``base_ptr`` (doubles)."""
    return base_ptr + 8 * field


DP_BETA = [
    [1 / 5],
    [3 / 40, 9 / 40],
    [44 / 45, -56 / 15, 32 / 9],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
    [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
]
DP_C_ERR = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720,
            -2187 / 6784 - -12231 / 42400, 11 / 84 - 649 / 6300, -1. / 60.]

TABLEAU = {
    "euler": dict(beta=[], c_sol=[1.0]),
    "rk4": dict(beta=[[1 / 3], [-1 / 3, 1.0], [1.0, -1.0, 1.0]], c_sol=[1 / 8, 3 / 8, 3 / 8, 1 / 8]),
    "dopri5": dict(beta=DP_BETA, c_sol=None),
    # the initial-step probe of dopri5: f(y0 + h0 f0) as "stage 1" of a two-stage table (f0 = stage 0 is in place)
    "probe": dict(beta=[[1.0]], c_sol=None),
}

# A/B switches, on unless the variable is "0".  A solver copies them into attributes of the same (lower-case) name when
# it is constructed; assigning the attribute on an instance before its first solve overrides the environment.
#   NLBAC_NORM_DEFER          the two norms that open a dopri5 solve without their elections (ode_dopri: _norm_defer_ok)
#   NLBAC_NORM_DEFER_ATTEMPT  ... and the attempts' error norm as tile partials + nlbac_dopri_control_tiles
#   NLBAC_INTERP_FOLD         the interpolation at t_end inside the attempt launches (ode_dopri: _interp_fold)
#   NLBAC_FIT_WORDS           activation rows AND ReLU mask words for solves that want weight gradients
#                             (odeint._fit_words_on, ode_traj.AffineTraj)
_ENV = dict(norm_defer="NLBAC_NORM_DEFER", norm_defer_attempt="NLBAC_NORM_DEFER_ATTEMPT",
            interp_fold="NLBAC_INTERP_FOLD", fit_words="NLBAC_FIT_WORDS")


def env_switch(name):
    return os.environ.get(_ENV[name], "1") != "0"


NORM_DEFER_ATTEMPT = env_switch("norm_defer_attempt")
