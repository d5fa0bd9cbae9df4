"""Host-side checks of ``nlbac_amd.rollout.rollout``: bad models, shapes, dtypes, devices and step sizes are refused
before anything is launched (no GPU needed)."""
import pytest
import torch


def model(kind):
    from nlbac_amd.sac_cbf_clf.model import NeuralODEModel
    return NeuralODEModel(3, 3, 6) if kind == "affine" else NeuralODEModel(12, 10)


def test_rollout_refuses_foreign_modules():
    from nlbac_amd.rollout import rollout
    with pytest.raises(TypeError):
        rollout(torch.nn.Linear(5, 3), torch.zeros(4, 3), torch.zeros(2, 4, 2), 0.02)


@pytest.mark.parametrize("kind,ns,nc", [("affine", 3, 2), ("concat", 10, 2)])
def test_rollout_validates_before_launching(kind, ns, nc):
    from nlbac_amd.rollout import rollout
    m = model(kind)
    x0, c = torch.zeros(4, ns), torch.zeros(2, 4, nc)
    bad = [
        (ValueError, dict(x0=torch.zeros(4, ns + 1))),
        (ValueError, dict(x0=torch.zeros(4))),
        (ValueError, dict(controls=torch.zeros(0, 4, nc))),
        (ValueError, dict(controls=torch.zeros(2, 5, nc))),
        (ValueError, dict(controls=torch.zeros(2, 4, nc + 1))),
        (ValueError, dict(controls=torch.zeros(4, nc))),
        (TypeError, dict(x0=torch.zeros(4, ns, dtype=torch.float64))),
        (TypeError, dict(controls=[[0.0]])),
        (TypeError, dict(dt=torch.tensor(0.02))),
        (TypeError, dict(dt=True)),
        (ValueError, dict(dt=0.0)),
        (ValueError, dict(dt=-0.02)),
        (ValueError, dict(dt=float("nan"))),
        (ValueError, dict(method="adams")),
        (ValueError, dict()),             # CPU tensors: a CUDA device is required
    ]
    for exc, kw in bad:
        args = dict(x0=x0, controls=c, dt=0.02, method="rk4")
        args.update(kw)
        with pytest.raises(exc):
            rollout(m, args["x0"], args["controls"], args["dt"], method=args["method"])


def test_one_launch_switch_reads_the_environment():
    import importlib
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import nlbac_amd.rollout as R; print(R.ONE_LAUNCH)"
    for val, want in (("0", "False"), ("1", "True")):
        env = dict(os.environ, NLBAC_ROLLOUT_ONE_LAUNCH=val)
        r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import nlbac_amd; " % root + code],
                           env=env, capture_output=True, text=True, timeout=120)
        assert r.stdout.strip().splitlines()[-1] == want, r.stderr[-2000:]
    assert importlib.import_module("nlbac_amd.rollout").METHODS == ("euler", "rk4", "dopri5")
