"""rlao_amd._lib.call: the one way into libaoenv, driven with a fake owner whose library records what it is handed (no GPU, no
shared library)."""
import ctypes as C

import numpy as np
import pytest
import torch

from rlao_amd import _lib as L


class _Lib:
    """Records the arguments of every entry point; ``aoenv_poke`` writes through its first pointer, ``aoenv_fail`` refuses."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("aoenv_"):
            raise AttributeError(name)

        def entry(h, *args):
            self.calls.append((name, h, args))
            if name == "aoenv_poke":
                C.cast(args[0], C.POINTER(C.c_double))[1] = 42.0
            if name == "aoenv_answer":
                return 7
            return 3 if name == "aoenv_fail" else 0
        return entry

    def aoenv_last_error(self):
        return b"the fake library says no"


class _Owner:
    def __init__(self):
        self.lib, self.h = _Lib(), C.c_void_p(0x1234)


def test_every_kind_of_argument_arrives_in_its_form():
    o = _Owner()
    cfg = L.AoModal(n_modes=3)
    arr = np.arange(6, dtype=np.float64).reshape(2, 3)
    t = torch.arange(4, dtype=torch.float32)
    out = C.c_int(0)
    ready = C.c_void_p(99)
    ref = C.byref(out)
    L.call(o, "aoenv_anything", None, cfg, arr, t, torch.empty((2, 0, 3)), 5, 0.25, ref, ready, True)
    (name, h, a), = o.lib.calls
    assert name == "aoenv_anything" and h is o.h
    assert a[0] is None
    assert a[1]._obj is cfg                                        # byref(struct): the library reads the caller's struct
    assert isinstance(a[2], C.c_void_p) and a[2].value == arr.ctypes.data
    assert isinstance(a[3], C.c_void_p) and a[3].value == t.data_ptr()
    assert a[4] is None                                            # an empty tensor has no address
    assert a[5] == 5 and type(a[5]) is int and a[6] == 0.25 and type(a[6]) is float
    assert a[7] is ref and a[8] is ready and a[9] is True          # ready-made ctypes objects and plain numbers: as they are


def test_a_stream_goes_as_a_plain_integer_and_no_arguments_is_fine():
    o = _Owner()
    L.call(o, "aoenv_measure", 0)
    L.call(o, "aoenv_profile")
    assert o.lib.calls == [("aoenv_measure", o.h, (0,)), ("aoenv_profile", o.h, ())]


def test_a_non_contiguous_array_is_refused_before_the_library_is_called():
    o = _Owner()
    a = np.zeros((4, 6))
    for bad in (a[:, ::2], a.T, np.asfortranarray(a)):
        with pytest.raises(ValueError, match="C-contiguous"):
            L.call(o, "aoenv_poke", bad, 0)
    assert o.lib.calls == []
    with pytest.raises(ValueError, match="C-contiguous"):
        L.address(a[:, ::2])
    L.call(o, "aoenv_upload", a[1:3], 0)                           # a contiguous window is the caller's memory too
    assert o.lib.calls[-1][2][0].value == a[1:3].ctypes.data


def test_the_array_handed_over_is_the_callers_own_memory():
    o = _Owner()
    buf = np.zeros(4)
    L.call(o, "aoenv_poke", buf)
    assert buf.tolist() == [0.0, 42.0, 0.0, 0.0]
    t = torch.zeros(4, dtype=torch.float64)
    L.call(o, "aoenv_poke", t)
    assert t.tolist() == [0.0, 42.0, 0.0, 0.0]


def test_a_status_other_than_zero_raises_with_the_librarys_message():
    o = _Owner()
    with pytest.raises(L.AoEnvError, match="the fake library says no"):
        L.call(o, "aoenv_fail", 1)
    assert o.lib.calls[-1][0] == "aoenv_fail"
    assert L.invoke(o, "aoenv_answer") == 7                        # an entry that answers instead of reporting: no check
    assert L.invoke(o, "aoenv_fail") == 3


def test_address_is_the_same_memory_as_an_integer():
    arr, t = np.zeros(3), torch.zeros(3)
    assert L.address(None) is None and L.address(torch.empty(0)) is None
    assert L.address(arr) == arr.ctypes.data and L.address(t) == t.data_ptr()
    cfg = L.AoModal(n_modes=1, h_m2c=L.address(arr), h_cm=None)
    assert cfg.h_m2c == arr.ctypes.data and cfg.h_cm is None
