"""The entry points of the fused backprop through rk4 and dopri5 solves of the GAT ODE function (csrc/gat_small.hip:
gode_gat_small_close_stages_f32; csrc/gat_driver.hip: gode_gat_ode_rk4_forward_save / _rk4_backprop /
_dopri5_step_backprop): they exist and return their validation codes before any HIP call (no GPU needed)."""
import ctypes

from graph_odenet_amd import _lib

NULLPTR, SHAPE, UNSUPPORTED = -1, -2, -5
P = ctypes.addressof


def _buf(n=64):
    """A host array standing in for a device pointer: validation never dereferences it."""
    return (ctypes.c_float * n)()


def _structs(n=37, d=16, heads=1, small_part=True):
    """A gode_gat_odefunc_t / gode_gat_workspace_t pair with every pointer the adjoint step wants set (to host memory)."""
    keep = [_buf() for _ in range(8)]
    a = P(keep[0])
    fs, ws = _lib.GatOdeFunc(), _lib.GatWorkspace()
    for g in (fs.mt, fs.ms_inc, fs.mt_inc):
        g.rowptr = a
    fs.src, fs.tgt, fs.n_edges = a, a, 600
    fs.n, fs.d, fs.groups, fs.eps_gn, fs.eps, fs.heads = n, d, min(32, d) if d > 0 else 1, 1e-5, 1e-6, heads
    for name in ("Wsrc", "Wtgt", "Wlog", "bf", "bw", "gamma", "beta"):
        setattr(fs, name, a)
    for name in ("X", "Ps", "Pt", "A2", "a", "amax", "wgt", "den", "logits_scratch", "dz", "da", "dPs", "dPt", "dA2", "pair", "gp",
                 "bp", "maxpath_scratch", "colsum_scratch", "colsum_scratch2", "zeros", "heads_scratch"):
        setattr(ws, name, a)
    for j in range(3):
        ws.wp[j] = a
    ws.small_part = a if small_part else None
    return fs, ws, keep


def test_symbols_exist():
    lib = _lib.load()
    for name in ("gode_gat_small_close_stages_f32", "gode_gat_ode_rk4_forward_save", "gode_gat_ode_rk4_backprop",
                 "gode_gat_ode_dopri5_step_backprop"):
        assert hasattr(lib, name), name
    assert _lib.CONSTANTS["GODE_PROF_GAT_STEP_CLOSE"] == 11
    assert lib.gode_abi_version() == 1


def test_close_stages_validation_codes():
    f = _lib.load().gode_gat_small_close_stages_f32
    b = [_buf() for _ in range(2)]
    ts = (ctypes.c_float * 7)()

    def args(n=37, d=16, heads=1, q=4):
        return [P(b[0]), n, d, heads, q, ts, P(b[1]), None]
    for i in (0, 5, 6):
        a = args()
        a[i] = None
        assert f(*a) == NULLPTR, i
    assert f(*args(q=0)) == SHAPE
    assert f(*args(q=8)) == SHAPE
    assert f(*args(q=-1)) == SHAPE
    assert f(*args(n=0)) == SHAPE
    assert f(*args(d=0)) == SHAPE
    assert f(*args(d=128)) == UNSUPPORTED
    assert f(*args(d=24)) == UNSUPPORTED
    assert f(*args(n=65537)) == UNSUPPORTED
    assert f(*args(d=64, heads=9)) == UNSUPPORTED
    assert f(*args(d=64, heads=3)) == UNSUPPORTED                       # heads do not divide d


def _forward_save_args(fs, ws, b, steps=(4, 0, 4)):
    return [ctypes.byref(fs), P(b[0]), P(b[1]), P(b[2]), ctypes.byref(ws), 0.0, 1.0, steps[0], steps[1], steps[2], None]


def test_rk4_forward_save_validation_codes():
    f = _lib.load().gode_gat_ode_rk4_forward_save
    b = [_buf() for _ in range(3)]
    fs, ws, _k = _structs()
    for i in (0, 1, 2, 3, 4):
        a = _forward_save_args(fs, ws, b)
        a[i] = None
        assert f(*a) == NULLPTR, i
    for steps in ((0, 0, 0), (4, -1, 2), (4, 0, 5), (4, 2, 2), (4, 3, 2)):
        assert f(*_forward_save_args(fs, ws, b, steps)) == SHAPE, steps
    fs0, ws0, _k0 = _structs(n=0)
    assert f(*_forward_save_args(fs0, ws0, b)) == SHAPE
    fs3, ws3, _k3 = _structs(d=64, heads=3)
    assert f(*_forward_save_args(fs3, ws3, b)) == SHAPE                 # heads do not divide d
    fs1, ws1, _k1 = _structs(d=128)
    assert f(*_forward_save_args(fs1, ws1, b)) == UNSUPPORTED
    fs2, ws2, _k2 = _structs(n=70000)
    assert f(*_forward_save_args(fs2, ws2, b)) == UNSUPPORTED
    fs4, ws4, _k4 = _structs(small_part=False)
    assert f(*_forward_save_args(fs4, ws4, b)) == UNSUPPORTED
    fs5, ws5, _k5 = _structs()
    ws5.dPs = None                                                       # a workspace without the adjoint's arrays
    assert f(*_forward_save_args(fs5, ws5, b)) == NULLPTR
    fs6, ws6, _k6 = _structs()
    fs6.Wlog = None
    assert f(*_forward_save_args(fs6, ws6, b)) == NULLPTR


def _ptr_array(bufs):
    return (ctypes.c_void_p * len(bufs))(*[P(x) if x is not None else None for x in bufs])


def _rk4_backprop_args(fs, ws, b, yb, steps=(4, 0, 4)):
    return [ctypes.byref(fs), P(b[0]), P(b[1]), P(b[2]), _ptr_array(yb), P(b[3]), P(b[4]), ctypes.byref(ws), 0.0, 1.0,
            steps[0], steps[1], steps[2], None]


def test_rk4_backprop_validation_codes():
    f = _lib.load().gode_gat_ode_rk4_backprop
    b = [_buf() for _ in range(5)]
    yb = [_buf() for _ in range(4)]
    fs, ws, _k = _structs()
    for i in (0, 1, 2, 3, 4, 5, 6, 7):
        a = _rk4_backprop_args(fs, ws, b, yb)
        a[i] = None
        assert f(*a) == NULLPTR, i
    assert f(*_rk4_backprop_args(fs, ws, b, yb[:2] + [None] + yb[3:])) == NULLPTR
    for steps in ((0, 0, 0), (4, -1, 2), (4, 0, 5), (4, 2, 2)):
        assert f(*_rk4_backprop_args(fs, ws, b, yb, steps)) == SHAPE, steps
    assert f(*_rk4_backprop_args(fs, ws, b, [yb[0], yb[1], yb[1], yb[3]])) == SHAPE        # two Ybar share an array
    assert f(*_rk4_backprop_args(fs, ws, b, [yb[0], b[1], yb[2], yb[3]])) == SHAPE         # a Ybar is the cotangent itself
    assert f(*_rk4_backprop_args(fs, ws, b, [yb[0], yb[1], yb[2], b[3]])) == SHAPE         # a Ybar is k_scratch
    fs1, ws1, _k1 = _structs(d=128)
    assert f(*_rk4_backprop_args(fs1, ws1, b, yb)) == UNSUPPORTED
    fs2, ws2, _k2 = _structs(d=64, heads=8, small_part=False)
    assert f(*_rk4_backprop_args(fs2, ws2, b, yb)) == UNSUPPORTED
    fs3, ws3, _k3 = _structs(d=0)
    assert f(*_rk4_backprop_args(fs3, ws3, b, yb)) == SHAPE


def _dopri5_args(fs, ws, b, k, yb, first=0, kbar7=True, kbar1=True):
    wk = (ctypes.c_double * 7)(*[0.1] * 7)
    return [ctypes.byref(fs), P(b[0]), _ptr_array(k), P(b[1]), P(b[2]) if kbar7 else None, 1.0, wk, 0.25, 0.125, first,
            _ptr_array(yb), P(b[3]), P(b[4]) if kbar1 else None, P(b[5]), P(b[6]), P(b[7]), ctypes.byref(ws), None]


def test_dopri5_step_backprop_validation_codes():
    f = _lib.load().gode_gat_ode_dopri5_step_backprop
    b = [_buf() for _ in range(8)]
    k = [_buf() for _ in range(7)]
    yb = [_buf() for _ in range(7)]
    fs, ws, _k = _structs(d=32, heads=4)
    for i in (0, 1, 2, 3, 6, 10, 11, 13, 14, 15, 16):
        a = _dopri5_args(fs, ws, b, k, yb)
        a[i] = None
        assert f(*a) == NULLPTR, i
    assert f(*_dopri5_args(fs, ws, b, k, yb, first=0, kbar1=False)) == NULLPTR            # kbar1 is a result unless first
    assert f(*_dopri5_args(fs, ws, b, k[:6] + [None], yb)) == NULLPTR
    assert f(*_dopri5_args(fs, ws, b, k, yb[:3] + [None] + yb[4:])) == NULLPTR
    assert f(*_dopri5_args(fs, ws, b, k, [None] + yb[1:], first=1)) == NULLPTR            # Ybar_1 is wanted when first
    assert f(*_dopri5_args(fs, ws, b, k, yb[:5] + [b[1]] + yb[6:])) == SHAPE              # a Ybar is g
    assert f(*_dopri5_args(fs, ws, b, k, yb[:5] + [b[3]] + yb[6:])) == SHAPE              # a Ybar is ybar_n
    assert f(*_dopri5_args(fs, ws, b, k, yb[:5] + [yb[6]] + yb[6:])) == SHAPE             # two Ybar share an array
    fs1, ws1, _k1 = _structs(d=128, heads=8)
    assert f(*_dopri5_args(fs1, ws1, b, k, yb)) == UNSUPPORTED
    assert f(*_dopri5_args(fs1, ws1, b, k, [None] + yb[1:], first=0, kbar7=False)) == UNSUPPORTED
    fs2, ws2, _k2 = _structs(d=32, heads=4, small_part=False)
    assert f(*_dopri5_args(fs2, ws2, b, k, yb, first=1, kbar1=False)) == UNSUPPORTED
    fs3, ws3, _k3 = _structs(n=-5, d=32, heads=4)
    assert f(*_dopri5_args(fs3, ws3, b, k, yb)) == SHAPE


def test_field_switch_and_members():
    from graph_odenet_amd import gat_ode, solver
    assert gat_ode.GatOdeField.BACKPROP_FUSED is True
    for name in ("rk4_forward_save", "rk4_backprop", "dopri5_step_backprop", "dopri5_backprop_work", "packed_grads",
                 "packed_param_grads"):
        assert getattr(gat_ode.GatOdeField, name) is None and getattr(solver.Field, name) is None, name
    assert callable(gat_ode.theta_param_grads)
