"""Constants of the NODE solvers (``odeint.py``): the Butcher tableaus and the environment switches."""
import os

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
#   NLBAC_NORM_DEFER          the two norms that open a dopri5 solve without their elections (odeint._norm_defer_ok)
#   NLBAC_NORM_DEFER_ATTEMPT  ... and the attempts' error norm as tile partials + nlbac_dopri_control_tiles
#   NLBAC_INTERP_FOLD         the interpolation at t_end inside the attempt launches (odeint._interp_fold)
#   NLBAC_FIT_WORDS           activation rows AND ReLU mask words for solves that want weight gradients
#                             (odeint._fit_words_on, rollout._Traj)
_ENV = dict(norm_defer="NLBAC_NORM_DEFER", norm_defer_attempt="NLBAC_NORM_DEFER_ATTEMPT",
            interp_fold="NLBAC_INTERP_FOLD", fit_words="NLBAC_FIT_WORDS")


def env_switch(name):
    return os.environ.get(_ENV[name], "1") != "0"


NORM_DEFER_ATTEMPT = env_switch("norm_defer_attempt")
