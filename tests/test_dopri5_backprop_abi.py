"""Argument validation of gode_gcn_ode_dopri5_step_backprop (csrc/ode_driver.hip): the codes come back before any HIP
call, so they are checked without a GPU.  Pointers that must never be dereferenced are dummies."""
import ctypes

from graph_odenet_amd import _lib

E_NULLPTR, E_SHAPE = -1, -2


def P(v):
    return ctypes.c_void_p(v)


def seven(base, holes=()):
    return (ctypes.c_void_p * 7)(*[None if i in holes else base + 256 * i for i in range(7)])


def call(f=True, y=P(256), k=None, g=P(512), kbar7=None, wk=True, first=0, ybar=None, ybar_n=P(768), kbar1=P(1024),
         theta=P(1280), ktheta=None, ws=None, n=8, d=16, groups=0):
    lib = _lib.load()
    fs = _lib.GcnOdeFunc()
    fs.n, fs.d, fs.groups, fs.eps = n, d, groups, 1e-5
    w = _lib.Rk4Workspace() if ws is None else ws
    return lib.gode_gcn_ode_dopri5_step_backprop(
        ctypes.byref(fs) if f else None, y, seven(1 << 16) if k is None else k, g, kbar7, 1.0,
        (ctypes.c_double * 7)(*[0.1] * 7) if wk else None, 0.0, 0.25, first, seven(1 << 17) if ybar is None else ybar,
        ybar_n, kbar1, theta, seven(1 << 18) if ktheta is None else ktheta, ctypes.byref(w), None, None)


def full_workspace():
    ws = _lib.Rk4Workspace()
    ws.dZ = ws.dS = ws.wpart = ws.colsum_scratch = 256
    return ws


def test_null_pointers():
    assert call(f=False) == E_NULLPTR
    assert call(y=None) == E_NULLPTR
    assert call(g=None) == E_NULLPTR
    assert call(wk=False) == E_NULLPTR
    assert call(ybar_n=None) == E_NULLPTR
    assert call(theta=None) == E_NULLPTR
    assert call(kbar1=None) == E_NULLPTR                         # needed unless the step opens an interval
    assert call(k=seven(1 << 16, holes=(6,))) == E_NULLPTR       # a stage derivative
    assert call(ktheta=seven(1 << 18, holes=(3,))) == E_NULLPTR
    assert call(ybar=seven(1 << 17, holes=(2,))) == E_NULLPTR
    assert call(ybar=seven(1 << 17, holes=(0,)), first=1, kbar1=None) == E_NULLPTR      # Ybar_1's buffer, first step only
    assert call(ybar=seven(1 << 17, holes=(0,))) == E_NULLPTR    # past the argument checks: the empty workspace
    assert call(ws=_lib.Rk4Workspace()) == E_NULLPTR
    ws = full_workspace()
    ws.wpart = None
    assert call(ws=ws) == E_NULLPTR
    assert call(ws=full_workspace(), groups=4) == E_NULLPTR      # GroupNorm without its partial buffers


def test_shapes_and_aliases():
    assert call(n=0) == E_SHAPE
    assert call(d=-1) == E_SHAPE
    assert call(ybar_n=P(512)) == E_SHAPE                        # ybar_n is g
    assert call(kbar7=P(1024)) == E_SHAPE                        # kbar1 is kbar7
    assert call(kbar7=P(768)) == E_SHAPE                         # ybar_n is kbar7
    assert call(g=P((1 << 17) + 256 * 4)) == E_SHAPE             # a Ybar work array is g
    assert call(kbar1=P(768)) == E_SHAPE                         # kbar1 is ybar_n
