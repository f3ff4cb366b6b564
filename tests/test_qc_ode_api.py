"""The continuous-depth edge-conditioned block of the QM9 models (qc_ode.py): names, signatures, state_dict keys,
drop-in exports, and the plain-torch path of EdgeODEfunc against a restatement of its formulas written here (no GPU).

RefEdgeODEfunc is the yardstick of tests/test_gpu_qc_ode.py too: it imports nothing from the code under test and holds
edge_data as an nn.Parameter, so that oracle/solver_ref's odeint_adjoint returns its gradient."""
import inspect
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F


class RefEdgeODEfunc(nn.Module):
    """f(t, x) = relu(Etgt . bmm(A, ([t | GN(x)] W)[Esrc]) + b), time column first."""

    def __init__(self, dim, Esrc, etgt, eval_, A, dtype=torch.float64):
        super().__init__()
        self.groups, self.eps = min(32, dim), 1e-5
        self.gamma, self.beta = nn.Parameter(torch.ones(dim, dtype=dtype)), nn.Parameter(torch.zeros(dim, dtype=dtype))
        self.W, self.b = nn.Parameter(torch.zeros(dim + 1, dim, dtype=dtype)), nn.Parameter(torch.zeros(dim, dtype=dtype))
        self.A = nn.Parameter(A.detach().clone().to(dtype))
        self.Esrc, self.etgt, self.val = Esrc.long(), etgt.long(), eval_.to(dtype)
        self.nfe = 0

    def load(self, func):
        """Parameters of an EdgeODEfunc-shaped state_dict (norm1.*, gc1.*)."""
        sd = {k: v.detach().cpu() for k, v in func.state_dict().items()}
        with torch.no_grad():
            self.gamma.copy_(sd["norm1.weight"]); self.beta.copy_(sd["norm1.bias"])
            self.W.copy_(sd["gc1.weight"]); self.b.copy_(sd["gc1.bias"])
        return self

    def forward(self, t, x):
        self.nfe += 1
        tt = torch.ones(x.shape[0], 1, dtype=x.dtype) * t
        xx = torch.cat([tt, F.group_norm(x, self.groups, self.gamma, self.beta, self.eps)], 1)
        S = torch.mm(xx, self.W)
        msg = torch.bmm(self.A, S.index_select(0, self.Esrc).unsqueeze(-1)).squeeze(-1)
        M = torch.zeros(x.shape[0], self.W.shape[1], dtype=x.dtype).index_add_(0, self.etgt, self.val.unsqueeze(1) * msg)
        return F.relu(M + self.b)


def small_batch(h, seed=0, n=11, E=30, dtype=torch.float64):
    """A batch with an atom that is no edge's target (the last), a duplicated (src, tgt) pair and non-unit values."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (E,), generator=g)
    tgt = torch.randint(0, n - 1, (E,), generator=g)
    src[1], tgt[1] = src[0], tgt[0]
    val = (torch.rand(E, generator=g) + 0.5).to(dtype)          # float32-representable: prepared edges keep float32 values
    A = torch.randn(E, h, h, generator=g, dtype=dtype) / h ** 0.5
    x = torch.randn(n, h, generator=g, dtype=dtype)
    return src, tgt, val, A, x


def randomise(func, seed=1):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in func.parameters():
            p.copy_(torch.rand(p.shape, generator=g, dtype=p.dtype) - 0.5)
        func.norm1.weight.add_(1.0)
    return func


def test_names_signatures_and_state_dict_keys():
    from graph_odenet_amd import qc_models, qc_ode
    assert qc_models.EdgeODEfunc is qc_ode.EdgeODEfunc and qc_models.EdgeODEBlock is qc_ode.EdgeODEBlock
    f = qc_ode.EdgeODEfunc(16)
    assert set(f.state_dict()) == {"norm1.weight", "norm1.bias", "gc1.weight", "gc1.bias"}
    assert f.norm1.num_groups == 16 and tuple(f.gc1.weight.shape) == (17, 16) and f.nfe == 0
    assert qc_ode.EdgeODEfunc(64).norm1.num_groups == 32
    sig = inspect.signature(qc_ode.EdgeODEBlock.__init__)
    assert list(sig.parameters)[1:] == ["odefunc", "tol", "method", "step_size", "adjoint"]
    assert [sig.parameters[k].default for k in ("tol", "method", "step_size", "adjoint")] == [1e-5, None, None, True]
    b = qc_ode.EdgeODEBlock(f)
    assert set(b.state_dict()) == {"odefunc." + k for k in f.state_dict()}
    b.nfe = 3
    assert f.nfe == 3 and b.nfe == 3
    assert list(inspect.signature(qc_ode.EdgeODEfunc.set_edges).parameters)[1:] == ["Esrc", "Etgt", "edge_data"]


@pytest.mark.parametrize("name", ["EdgeODE1_K_Sum", "EdgeODE1_K_Set2Set"])
def test_models(name):
    from graph_odenet_amd import qc_models
    cls = getattr(qc_models, name)
    ref = inspect.signature(qc_models.EdgeRES1_K_Set2Set.__init__)
    assert str(inspect.signature(cls.__init__)) == str(ref)
    m = cls(node_features=13, edge_features=5, target_features=12, hidden_features=16, s2s_processing_steps=3, dropout=0.0,
            method="rk4", step_size=0.25, tol=1e-4, adjoint=False)
    assert (m.ode.method, m.ode.step_size, m.ode.tol, m.ode.adjoint) == ("rk4", 0.25, 1e-4, False)
    d = cls(node_features=13, edge_features=5, hidden_features=32)
    assert (d.ode.method, d.ode.step_size, d.ode.tol, d.ode.adjoint) == (None, None, 1e-5, True)
    tops = {k.split(".")[0] for k in m.state_dict()}
    assert tops == {"mlpin", "gcin", "ode", "gcout", "mlpout", "ee"} | ({"s2s"} if name.endswith("Set2Set") else set())
    assert {k for k in m.state_dict() if k.startswith("ode.")} == {"ode.odefunc." + k for k in
                                                                    ("norm1.weight", "norm1.bias", "gc1.weight", "gc1.bias")}
    with pytest.raises(ValueError, match="divisible"):         # GroupNorm(32, 73): torch's own refusal, as in RESKnorm
        cls(node_features=13, edge_features=5)


def test_dropin_exports_and_unimplemented_model_stays():
    from graph_odenet_amd import qc_models
    d = os.path.join(os.path.dirname(os.path.abspath(qc_models.__file__)), "dropin", "QC")
    sys.path.insert(0, d)
    try:
        sys.modules.pop("layer_models", None)
        import layer_models
        assert layer_models.EdgeODE1_K_Sum is qc_models.EdgeODE1_K_Sum
        assert layer_models.EdgeODE1_K_Set2Set is qc_models.EdgeODE1_K_Set2Set
        with pytest.raises(NotImplementedError):
            layer_models.UnimplementedModel()
    finally:
        sys.path.remove(d)
        sys.modules.pop("layer_models", None)


@pytest.mark.parametrize("form", ["dense", "sparse", "prepared"])
@pytest.mark.parametrize("h", [16, 64])
def test_cpu_forward_is_the_restatement(form, h):
    """On CPU tensors the fused hook declines and forward is plain torch: bit for bit the restatement in float64."""
    from graph_odenet_amd import qc_layers, qc_ode
    src, tgt, val, A, x = small_batch(h)
    n, E = x.shape[0], src.numel()
    f = randomise(qc_ode.EdgeODEfunc(h).double())
    dense = torch.zeros(n, E, dtype=torch.float64)
    dense[tgt, torch.arange(E)] = val
    Etgt = {"dense": lambda: dense, "sparse": lambda: dense.to_sparse(),
            "prepared": lambda: qc_layers.prepared_edges(src, tgt, n, val)}[form]()
    A = A.clone().requires_grad_(True)
    f.set_edges(src, Etgt, A)
    assert f.gode_fields(x) is None
    assert f.gode_extra_inputs() == (A,)
    ref = RefEdgeODEfunc(h, src, tgt, val, A).load(f)
    t = torch.tensor(0.375, dtype=torch.float64)
    got, want = f(t, x), ref(t, x)
    assert torch.equal(got, want)
    assert f.nfe == 1 and (got[-1] == F.relu(f.gc1.bias)).all()       # the last atom receives no message
    R = torch.randn(got.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    gA, = torch.autograd.grad((got * R).sum(), A)
    gAr, = torch.autograd.grad((want * R).sum(), ref.A)
    assert torch.allclose(gA, gAr, rtol=1e-12, atol=1e-12)
