"""Argument validation of the backprop entry points (csrc/ode_driver.hip, backprop.hip, small.hip, spmm.hip): the codes
come back before any HIP call, so they are checked without a GPU.  Pointers that must never be dereferenced are dummies."""
import ctypes

from graph_odenet_amd import _lib

E_NULLPTR, E_SHAPE, E_RANGE = -1, -2, -4
DUMMY = ctypes.c_void_p(256)          # a non-NULL device address the validation never touches


def structs(n=8, d=16):
    f = _lib.GcnOdeFunc()
    f.n, f.d, f.groups, f.eps = n, d, 0, 1e-5
    ws = _lib.Rk4Workspace()
    return f, ws


def test_forward_save_validation():
    lib = _lib.load()
    f, ws = structs()
    fwd = lib.gode_gcn_ode_rk4_forward_save
    assert fwd(None, DUMMY, DUMMY, DUMMY, ctypes.byref(ws), 0.0, 1.0, 4, 0, 4, None) == E_NULLPTR
    assert fwd(ctypes.byref(f), DUMMY, None, DUMMY, ctypes.byref(ws), 0.0, 1.0, 4, 0, 4, None) == E_NULLPTR
    assert fwd(ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(ws), 0.0, 1.0, 0, 0, 1, None) == E_SHAPE     # no steps
    assert fwd(ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(ws), 0.0, 1.0, 4, 2, 2, None) == E_SHAPE     # empty range
    assert fwd(ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(ws), 0.0, 1.0, 4, 0, 5, None) == E_SHAPE     # past the grid
    assert fwd(ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(ws), 0.0, 1.0, 4, 0, 4, None) == E_NULLPTR   # ws->S
    f0, _ = structs(n=0)
    assert fwd(ctypes.byref(f0), DUMMY, DUMMY, DUMMY, ctypes.byref(ws), 0.0, 1.0, 4, 0, 4, None) == E_SHAPE


def test_backprop_validation():
    lib = _lib.load()
    f, ws = structs()
    res = ctypes.c_void_p()
    bp = lib.gode_gcn_ode_rk4_backprop
    assert bp(ctypes.byref(f), None, DUMMY, DUMMY, ctypes.byref(res), ctypes.byref(ws), None, 0.0, 1.0, 4, 0, 4, None) == E_NULLPTR
    assert bp(ctypes.byref(f), DUMMY, DUMMY, DUMMY, None, ctypes.byref(ws), None, 0.0, 1.0, 4, 0, 4, None) == E_NULLPTR
    assert bp(ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(res), ctypes.byref(ws), None, 0.0, 1.0, 4, 3, 1, None) == E_SHAPE
    assert bp(ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(res), ctypes.byref(ws), None, 0.0, 1.0, 4, 0, 4, None) == E_NULLPTR
    for i in range(4):                                           # stage buffers given, the partial buffers still missing
        ws.ka[i] = ws.ktheta[i] = 256
    ws.dZ = ws.dS = 256
    assert bp(ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(res), ctypes.byref(ws), None, 0.0, 1.0, 4, 0, 4, None) == E_NULLPTR


def test_masked_cotangent_validation():
    lib = _lib.load()
    lc = _lib.LinComb()
    assert lib.gode_masked_cot_f32(ctypes.byref(lc), DUMMY, DUMMY, -1, 16, None, None) == E_SHAPE
    assert lib.gode_masked_cot_f32(ctypes.byref(lc), None, DUMMY, 8, 16, None, None) == E_NULLPTR
    assert lib.gode_masked_cot_f32(ctypes.byref(lc), DUMMY, DUMMY, 8, 16, None, None) == E_RANGE       # no terms
    lc.n, lc.coef[0], lc.ptr[0] = 1, 1.0, 256
    assert lib.gode_masked_cot_f32(ctypes.byref(lc), DUMMY, DUMMY, 8, 16, None, None) == E_SHAPE       # dZ is a term
    assert lib.gode_masked_cot_parts(2708, 64) == -(-2708 // (16 * 16))
    assert lib.gode_masked_cot_parts(1 << 20, 128) == (1 << 20) // 128
    assert lib.gode_masked_cot_parts(100, 6) == 0                                                     # no 16-byte kernel


def test_save_variants_validation():
    lib = _lib.load()
    f, _ = structs()
    lc = _lib.LinComb()
    assert lib.gode_spmm_csr_save_f32(None, None, None, None, 0, None, 0, None, None, 4, None, 4, 3, 8, None, DUMMY, None) == E_SHAPE
    assert lib.gode_spmm_csr_save_f32(DUMMY, DUMMY, None, None, 0, None, 0, None, DUMMY, 8, DUMMY, 8, 3, 8, None, None, None) == E_NULLPTR
    assert lib.gode_gcn_feval_small_save_f32(ctypes.byref(f), ctypes.byref(lc), 0.0, 1.0, None, DUMMY, None, None) == E_NULLPTR
    assert lib.gode_gcn_feval_small_save_f32(ctypes.byref(f), ctypes.byref(lc), 0.0, 1.0, None, DUMMY, DUMMY, None) == E_SHAPE
    assert lib.gode_gcn_vjp_small_next_f32(ctypes.byref(f), ctypes.byref(lc), DUMMY, 1.0, None, DUMMY, DUMMY,
                                           ctypes.byref(lc), DUMMY, None, None) == E_NULLPTR
    nxt = _lib.LinComb()
    nxt.n, nxt.coef[0], nxt.ptr[0] = 1, 1.0, 512
    assert lib.gode_gcn_vjp_small_next_f32(ctypes.byref(f), ctypes.byref(lc), DUMMY, 1.0, None, DUMMY, DUMMY,
                                           ctypes.byref(nxt), DUMMY, DUMMY, None) == E_SHAPE         # dZ_next is dZ
