"""The entry points of csrc/edge_backprop.hip (fused backprop through solves over the edge-conditioned ODE function): they
exist, report the shapes they support, and return their validation codes before any HIP call (no GPU needed)."""
import ctypes

from graph_odenet_amd import _lib

NULLPTR, SHAPE, RANGE, UNSUPPORTED = -1, -2, -4, -5


def _buf(n=64):
    """A host array standing in for a device pointer: validation never dereferences it."""
    return (ctypes.c_float * n)()


def _lc(ptrs, n=None):
    lc = _lib.LinComb()
    lc.n = len(ptrs) if n is None else n
    for j, p in enumerate(ptrs):
        lc.coef[j] = 1.0
        lc.ptr[j] = ctypes.addressof(p)
    return lc


def _stage_args(h=96, groups=32, n_rows=11, cot=None, yin=None, outs=None, k=None):
    b = [_buf() for _ in range(16)]
    cot = cot if cot is not None else _lc(b[0:3])
    yin = yin if yin is not None else _lc(b[3:6])
    outs = outs if outs is not None else b[6:12]
    p = ctypes.addressof
    return [p(b[12]), None, p(b[13]), None, p(b[14]), ctypes.byref(cot), 0.5, p(k if k is not None else b[15]),
            ctypes.byref(yin), 0.25, p(b[12]), p(b[13]), p(b[14]), groups, 1e-5, h, n_rows, 30] + [p(o) for o in outs] + [None]


def test_symbols_exist():
    lib = _lib.load()
    for name in ("gode_edge_ode_feval_save_f32", "gode_edge_ode_stage_bwd_f32", "gode_edge_ode_step_close_f32",
                 "gode_edge_ode_stage_bwd_supported"):
        assert hasattr(lib, name), name


def test_supported_shapes():
    lib = _lib.load()
    for shape in ((330, 96, 32), (330, 64, 32), (11, 7, 7)):
        assert lib.gode_edge_ode_stage_bwd_supported(*shape) == 1, shape
    assert lib.gode_edge_ode_stage_bwd_supported(330, 113, 113) == 0
    assert lib.gode_edge_ode_stage_bwd_supported(330, 64, 16) == 0          # 4 channels per group
    assert lib.gode_edge_ode_stage_bwd_supported(330, 96, 0) == 0


def test_stage_bwd_validation_codes():
    lib = _lib.load()
    f = lib.gode_edge_ode_stage_bwd_f32
    assert f(*_stage_args(h=0)) == SHAPE
    assert f(*_stage_args(h=-3)) == SHAPE
    assert f(*_stage_args(h=113, groups=113)) == RANGE
    b = [_buf() for _ in range(3)]
    assert f(*_stage_args(cot=_lc(b, n=9))) == RANGE                         # more than 8 terms
    assert f(*_stage_args(yin=_lc(b, n=9))) == RANGE
    args = _stage_args()
    args[5] = None
    assert f(*args) == NULLPTR                                               # no cotangent
    for i in (0, 7, 10, 12, 18, 19, 20, 21, 22):                             # rowptr, k, gamma, W, the five outputs
        args = _stage_args()
        args[i] = None
        assert f(*args) == NULLPTR, i
    lc = _lc(b)
    lc.ptr[1] = None
    assert f(*_stage_args(cot=lc)) == NULLPTR
    assert f(*_stage_args(h=96, groups=36)) == SHAPE                         # groups do not divide h
    assert f(*_stage_args(h=64, groups=16)) == UNSUPPORTED                   # 4 channels per group
    outs = [_buf() for _ in range(6)]
    for q in range(5):
        assert f(*_stage_args(cot=_lc([b[0], outs[q], b[1]]), outs=outs)) == SHAPE, "cotangent term aliases output %d" % q
    assert f(*_stage_args(yin=_lc([outs[2]]), outs=outs)) == SHAPE
    assert f(*_stage_args(k=outs[0], outs=outs)) == SHAPE
    assert f(*_stage_args(n_rows=0)) == 0                                    # nothing to do, nothing launched


def test_step_close_validation_codes():
    lib = _lib.load()
    f = lib.gode_edge_ode_step_close_f32
    b = [_buf() for _ in range(5)]

    def arr(q, fill):
        a = (ctypes.c_void_p * max(q, 1))()
        for i in range(q):
            a[i] = ctypes.addressof(fill)
        return a

    def args(q=4, h=96):
        return [q, arr(q, b[0]), arr(q, b[1]), arr(q, b[2]), arr(q, b[3]), (ctypes.c_float * max(q, 1))(), 11, 330, h,
                ctypes.addressof(b[4]), None]
    assert f(*args(q=9)) == RANGE                                            # more than 8 stages
    assert f(*args(q=0)) == RANGE
    assert f(*args(h=0)) == SHAPE
    assert f(*args(h=113)) == RANGE
    for i in (1, 2, 3, 4, 5, 9):
        a = args()
        a[i] = None
        assert f(*a) == NULLPTR, i
    a = args()
    a[2][3] = None                                                           # one stage's dM missing
    assert f(*a) == NULLPTR


def test_feval_save_validation_codes():
    lib = _lib.load()
    f = lib.gode_edge_ode_feval_save_f32
    b = [_buf() for _ in range(9)]
    p = ctypes.addressof
    good = [p(b[0]), None, None, p(b[1]), p(b[2]), p(b[3]), 96, 11, p(b[4]), None, 0.5, p(b[5]), p(b[6]), None]
    assert f(*(good[:6] + [0] + good[7:])) == SHAPE
    assert f(*(good[:6] + [113] + good[7:])) == RANGE
    assert f(*(good[:12] + [None, None])) == NULLPTR                         # no k
    assert f(*(good[:12] + [p(b[5]), None])) == SHAPE                        # k aliases out
    pre = _lc([b[7], b[6]])
    assert f(*(good[:9] + [ctypes.byref(pre)] + good[10:])) == SHAPE         # k aliases a pre term


def test_field_switch():
    from graph_odenet_amd import qc_ode
    assert qc_ode.EdgeOdeField.BACKPROP_FUSED is True
