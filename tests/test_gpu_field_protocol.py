"""The field protocol of solver.Field: every optional member defaults to "absent", so a field that defines `eval` alone
runs through both integrators, and the generic adjoint field (odeint.AutogradAdjointField) builds its own state and hands
back its own parameter gradients.  y' = -c y on an 8 x 4 state, against the closed form y(1) = exp(-c) y0."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def state(lo=0.5, hi=1.5, seed=0):
    """8 x 4 values away from zero, so that relative errors are taken element by element."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(8, 4, generator=g) * (hi - lo) + lo).to(DEV)


def rel_err(got, ref):
    return ((got.double() - ref.double()).abs() / ref.double().abs()).max().item()


def decay_field():
    from graph_odenet_amd import solver

    class Decay(solver.Field):
        def eval(self, t, terms, out):
            out[0].copy_(-sum(c * x for c, x in terms[0]))
    return Decay()


def test_eval_only_field_rk4():
    """16 steps of the 3/8 rule over [0, 1]: truncation ~1e-8 at h = 1/16, the rest is fp32 rounding."""
    from graph_odenet_amd import solver
    y0 = state()
    y = [y0.clone()]
    assert solver.integrate_rk4(decay_field(), y, 0.0, 1.0, 16) == 64
    err = rel_err(y[0], y0.double() * math.exp(-1.0))
    print("rk4 rel err %.3e" % err)
    assert err <= 1e-6


def test_eval_only_field_dopri5():
    from graph_odenet_amd import solver
    y0 = state()
    (y,), stats = solver.integrate_dopri5(decay_field(), [y0.clone()], 0.0, 1.0, 1e-6, 1e-6)
    err = rel_err(y, y0.double() * math.exp(-1.0))
    print("dopri5 rel err %.3e, %d accepted, %d rejected" % (err, stats.accepted, stats.rejected))
    assert stats.accepted >= 1 and err <= 1e-4


class Decay(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.c = torch.nn.Parameter(torch.tensor(c))

    def forward(self, t, y):
        return -self.c * y


@pytest.mark.parametrize("method", ["rk4", "dopri5"])
def test_generic_adjoint_matches_closed_form(method):
    from graph_odenet_amd import odeint as OI
    y0, R = state(seed=1), state(seed=2)
    f = Decay(0.8).to(DEV)
    x = y0.clone().requires_grad_(True)
    out = OI.odeint_adjoint(f, x, torch.tensor([0.0, 1.0]), rtol=1e-6, atol=1e-6, method=method,
                            options={"step_size": 1.0 / 16} if method == "rk4" else None)
    (out[1] * R).sum().backward()

    c = torch.tensor(0.8, dtype=torch.float64, requires_grad=True)
    x64 = y0.double().cpu().requires_grad_(True)
    (torch.exp(-c) * x64 * R.double().cpu()).sum().backward()
    e_y, e_x = rel_err(out[1].detach().cpu(), (torch.exp(-c) * x64).detach()), rel_err(x.grad.cpu(), x64.grad)
    e_c = abs(f.c.grad.item() - c.grad.item()) / abs(c.grad.item())
    print("%s: y(1) %.3e  dL/dy0 %.3e  dL/dc %.3e" % (method, e_y, e_x, e_c))
    assert e_y <= 1e-4 and e_x <= 1e-4 and e_c <= 1e-4
