"""The handle wrappers of graphem-rapids_amd/_native.py and the life cycle behind them (csrc/host_util.h), without a GPU: a
create that fails owns nothing, a refused budget changes nothing, close is idempotent and a closed handle refuses every call,
every exported symbol carries a ctypes signature, the create-time messages of two modules stay apart, and host-path handles
and a refused engine leave the count of live device allocations where it was."""
import numpy as np
import pytest

from graphem_rapids_amd import _native

COLS = [np.arange(8.0), np.arange(8.0)[::-1]]
NO_SUCH_DEVICE = 4096


@pytest.mark.parametrize("cls,args", [
    (_native.ICGraph, (4, [[0, 1]], False, NO_SUCH_DEVICE)),
    (_native.CentGraph, (4, [[0, 1]], NO_SUCH_DEVICE)),
    (_native.Generator, (NO_SUCH_DEVICE,)),
    (_native.Correlation, (COLS, NO_SUCH_DEVICE)),
])
def test_failed_create_raises_and_owns_no_handle(cls, args):
    obj = cls.__new__(cls)
    with pytest.raises(RuntimeError, match="invalid device ordinal 4096"):
        obj.__init__(*args)
    assert obj.handle.value is None
    obj.close()   # nothing to destroy


def _generator_calls(g):
    return [lambda: g.ba(50, 3, seed=1), lambda: g.sbm([6, 7], [[0.5, 0.2], [0.2, 0.9]], seed=2),
            lambda: g.geometric(40, 0.3, seed=3)]


def _correlation_calls(c):
    return [lambda: c.matrix(sums=True), lambda: c.bootstrap([[0, 1]], 5, seed=4, sums=True)]


def _flat(result):
    return [np.asarray(a) for a in (result if isinstance(result, tuple) else (result,))]


@pytest.mark.parametrize("make,calls", [(lambda: _native.Generator(-1), _generator_calls),
                                        (lambda: _native.Correlation(COLS, -1), _correlation_calls)])
def test_refused_budget_close_twice_and_calls_after_close(make, calls):
    obj = make()
    before = [_flat(call()) for call in calls(obj)]
    with pytest.raises(ValueError, match="budget must be >= 0"):
        obj.set_memory_budget(-1)
    for want, call in zip(before, calls(obj)):
        got = _flat(call())
        assert len(got) == len(want)
        for a, b in zip(want, got):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    obj.close()
    obj.close()
    assert obj.handle.value is None
    for call in calls(obj) + [lambda: obj.set_memory_budget(0), lambda: obj.set_memory_budget(-1)]:
        with pytest.raises(ValueError, match="handle is NULL"):
            call()


def test_every_symbol_has_a_signature():
    lib = _native.load()
    assert len(_native.SYMBOLS) == len(set(_native.SYMBOLS))
    for name in _native.SYMBOLS:
        fn = getattr(lib, name)
        restype, argtypes = _native.SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype, name


def test_create_messages_of_two_modules_stay_apart():
    lib = _native.load()
    with pytest.raises(ValueError, match=r"arc 0 has a vertex id outside \[0, n\)"):
        _native.ICGraph(10, [[0, 10]])
    with pytest.raises(ValueError, match=r"edge 1 has a vertex id outside \[0, n\)"):
        _native.CentGraph(5, [[0, 1], [2, 7]])
    assert lib.gh_ic_last_error(None).decode().startswith("arc 0 ")
    assert lib.gh_cent_last_error(None).decode().startswith("edge 1 ")


def test_host_path_handles_and_a_refused_engine_hold_no_device_allocation():
    """gh_debug_live_allocations counts what the library's handles hold on devices: a host-path handle (device_id = -1) of
    each kind, used and closed, and a gh_create that is refused (for its partition where there is a device, for the lack of
    one elsewhere) leave the count and the bytes unchanged."""
    start = _native.live_allocations()
    g = _native.Generator(-1)
    edges = g.ba(50, 3, seed=1)
    g.close()
    c = _native.Correlation(COLS, -1)
    c.matrix()
    c.close()
    q = _native.LayoutQuality(edges, 50, -1)
    q.set_positions(np.random.default_rng(0).standard_normal((50, 2)).astype(np.float32))
    q.crossings()
    q.close()
    p = _native.EdgeListParser(-1)
    p.parse(b"0 1\n1 2\n")
    p.close()
    with pytest.raises((ValueError, RuntimeError), match="partition out of range|no HIP device available"):
        _native.Engine(50, 2, edges, 1.0, 0.2, 0.5, 3, 8, partition=(10, 5, 0, 0))   # row_lo > row_hi
    assert _native.live_allocations() == start
