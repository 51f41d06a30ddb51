"""`_lib.call`, the one way the package calls an export of libgcr.so, against a stand-in handle: what each kind of argument
arrives as, what is refused before the function is entered, where the stream goes and what the return becomes.  No device
and no built library needed; tests/test_abi_cpu.py drives the same function through the real host planners."""
import ctypes
import types
from ctypes import c_double, c_float, c_int32, c_int64, c_uint64, c_void_p

import numpy as np
import pytest
import torch

from recommendation_amd import _lib

P = c_void_p
SIGNATURES = {
    "fk_launch_f32": (c_int32, [P, c_int64, c_float, P, c_uint64, c_double, P]),     # ..., void* stream
    "fk_plan_host": (c_int32, [P, c_int64, P]),                                      # no stream
    "fk_workspace_bytes": (c_int64, [c_int64, c_int32]),
    "fk_supported": (c_int32, [c_int32]),
}
STREAM = 0x5EED0


@pytest.fixture
def fake(monkeypatch):
    """A handle with SIGNATURES' exports as plain functions that record their arguments; `fake.ret` is the next return."""
    h = types.SimpleNamespace(seen=[], ret=0)

    def export(name):
        def fn(*args):
            h.seen.append((name, args))
            return h.ret
        return fn

    for name in SIGNATURES:
        setattr(h, name, export(name))
    monkeypatch.setattr(_lib, "_lib", h)
    monkeypatch.setattr(_lib, "_exports", _lib._bind(h, SIGNATURES))
    monkeypatch.setattr(_lib, "cur_stream", lambda device=None: c_void_p(STREAM + (device.index or 0 if device is not None else 0)))
    return h


def _value(a):
    return a.value if isinstance(a, c_void_p) else a


def test_bind_sets_the_prototypes_and_the_kinds(fake):
    (plain, streamed, status), fn = _lib._exports["fk_launch_f32"], fake.fk_launch_f32
    assert fn.restype is c_int32 and fn.argtypes == SIGNATURES["fk_launch_f32"][1]
    t = torch.zeros(3)
    assert plain(t, 1, 2.0, None, 3, 4.0, None) == (t.data_ptr(), 1, 2.0, None, 3, 4.0, None) and status
    assert streamed(None, 1, 2.0, t, 3, 4.0, "s") == (None, 1, 2.0, t.data_ptr(), 3, 4.0, "s")     # the stream passes through
    assert not _lib._exports["fk_workspace_bytes"][2]                 # an int64 is a value


def test_int32_answers_are_listed_by_name(monkeypatch):
    """An int32 return is a status code unless the export is in INT32_ANSWERS: the list holds real int32 exports, every
    *_supported query among them, and `_bind` treats exactly the listed ones as values."""
    assert len(set(_lib.INT32_ANSWERS)) == len(_lib.INT32_ANSWERS)
    for name in _lib.INT32_ANSWERS:
        assert _lib.SIGNATURES[name][0] is c_int32, name
    for name in _lib.SIGNATURES:
        if name.endswith("_supported"):
            assert name in _lib.INT32_ANSWERS, name
    h = types.SimpleNamespace(**{name: (lambda *a: 0) for name in ("gcr_version", "gcr_bitmap_set", "gcr_bt_supported")})
    sigs = {name: _lib.SIGNATURES[name] for name in vars(h)}
    table = _lib._bind(h, sigs)
    assert table["gcr_version"][0]() == ()
    assert [table[n][2] for n in ("gcr_version", "gcr_bitmap_set", "gcr_bt_supported")] == [False, True, False]


def test_pointer_and_numeric_slots_arrive_converted(fake):
    t = torch.arange(6, dtype=torch.float32)
    host = np.arange(4, dtype=np.int64)
    assert _lib.call("fk_launch_f32", t, 6, 0.5, None, 2 ** 64 - 1, 0.25, on=t) is None
    (name, args), = fake.seen
    assert name == "fk_launch_f32" and len(args) == 7
    assert args[0] == t.data_ptr() and args[3] is None                # a tensor as its data_ptr(), None as NULL
    assert args[1:3] == (6, 0.5) and args[4:6] == (2 ** 64 - 1, 0.25)
    assert _value(args[6]) == STREAM                                  # the stream last
    fake.seen.clear()
    _lib.call("fk_plan_host", host, np.int64(4), host[1:2])           # numpy arrays as their addresses, a numpy scalar
    (_, args), = fake.seen
    assert args == (host.ctypes.data, 4, host.ctypes.data + 8) and len(args) == 3        # ... and no stream without on=
    fake.seen.clear()
    _lib.call("fk_plan_host", c_void_p(1234), 1, None)                # a c_void_p as it is
    assert _value(fake.seen[0][1][0]) == 1234


def test_on_takes_a_tensor_a_device_or_a_stream_pointer(fake):
    t = torch.zeros(2)
    for on, want in ((t, STREAM), (torch.device("cuda", 3), STREAM + 3), (c_void_p(77), 77)):
        fake.seen.clear()
        _lib.call("fk_launch_f32", t, 2, 1.0, t, 0, 0.0, on=on)
        assert _value(fake.seen[0][1][-1]) == want and len(fake.seen[0][1]) == 7


def test_refused_before_the_function_is_entered(fake):
    t = torch.zeros(4, 4)
    with pytest.raises(_lib.GcrError, match="libgcr needs contiguous tensors"):
        _lib.call("fk_launch_f32", t.t(), 4, 1.0, None, 0, 0.0, on=t)
    with pytest.raises(_lib.GcrError, match="libgcr needs contiguous tensors"):
        _lib.call("fk_plan_host", np.zeros((4, 4), np.int64)[:, 0], 4, None)
    with pytest.raises(TypeError, match=r"fk_launch_f32: argument 1 is a number"):
        _lib.call("fk_launch_f32", t, torch.tensor(4), 1.0, None, 0, 0.0, on=t)          # a tensor in a numeric slot
    with pytest.raises(TypeError, match=r"fk_launch_f32: argument 2 is a number"):
        _lib.call("fk_launch_f32", t, 4, torch.tensor(1.0), None, 0, 0.0, on=t)
    with pytest.raises(TypeError, match=r"fk_launch_f32: argument 3 is a pointer"):
        _lib.call("fk_launch_f32", t, 4, 1.0, t.data_ptr(), 0, 0.0, on=t)                # a Python int in a pointer slot
    with pytest.raises(TypeError, match=r"fk_plan_host: argument 0 is a pointer"):
        _lib.call("fk_plan_host", 0, 4, None)
    with pytest.raises(TypeError, match=r"fk_launch_f32\(\) (takes|missing)"):
        _lib.call("fk_launch_f32", t, 4, 1.0, None, 0, 0.0)                              # the stream forgotten
    with pytest.raises(TypeError, match=r"fk_launch_f32\(\) (takes|missing)"):
        _lib.call("fk_launch_f32", t, 4, 1.0, None, 0, on=t)                             # an argument forgotten
    with pytest.raises(TypeError, match=r"fk_plan_host\(\) takes"):
        _lib.call("fk_plan_host", None, 4, None, on=t)                                   # a stream nobody asked for
    with pytest.raises(KeyError):
        _lib.call("fk_not_an_export")
    assert fake.seen == []


def test_status_codes_raise_under_the_exports_name(fake):
    t = torch.zeros(2)
    fake.ret = -1
    with pytest.raises(_lib.GcrError, match=r"fk_launch_f32: invalid or unsupported arguments \(code -1\)"):
        _lib.call("fk_launch_f32", t, 2, 1.0, None, 0, 0.0, on=t)
    fake.ret = -1003
    with pytest.raises(_lib.GcrError, match="fk_plan_host: HIP runtime error 3"):
        _lib.call("fk_plan_host", None, 0, None)


def test_queries_return_their_value(fake, monkeypatch):
    fake.ret = 5 << 32
    assert _lib.call("fk_workspace_bytes", 10, 64) == 5 << 32
    monkeypatch.setattr(_lib, "INT32_ANSWERS", _lib.INT32_ANSWERS + ("fk_supported",))
    monkeypatch.setattr(_lib, "_exports", _lib._bind(fake, SIGNATURES))
    fake.ret = -1                                                     # a listed int32 answer: handed back as it is
    assert _lib.call("fk_supported", 64) == -1
    fake.ret = 1000
    ws = _lib.workspace("fk_workspace_bytes", 10, 64, device="cpu")   # workspace() asks through call
    assert ws.numel() == 250 and fake.seen[-1] == ("fk_workspace_bytes", (10, 64))


def test_ctypes_refuses_a_wrong_count_too():
    """What `call` leans on below its own count check: with argtypes set, ctypes itself refuses a call that is short."""
    libc = ctypes.CDLL(None)
    libc.labs.restype, libc.labs.argtypes = ctypes.c_long, [ctypes.c_long]
    assert libc.labs(-3) == 3
    with pytest.raises(TypeError):
        libc.labs()
