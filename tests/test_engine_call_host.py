"""Host-side checks of engine.Handle.call and Handle.sized_workspace, the one place a C-ABI compute call is made from: what reaches
the C function for each kind of argument, and what each return code raises.  The library is a recording stand-in.  No GPU."""
import ctypes as C

import pytest
import torch

from torch_tts_amd import _lib
from torch_tts_amd import engine as E

H = 0x1234   # the handle
STREAM = 0x5678  # what the patched engine._stream answers
HIP_TEXT = "hipErrorLaunchFailure (the stand-in's)"


class Recorder:
    """In the library's place: every function records its arguments; ttsx_frob answers ``rc``, the size query ``nbytes``."""

    def __init__(self, rc=_lib.OK, nbytes=0):
        self.rc, self.nbytes, self.calls = rc, nbytes, []

    def ttsx_frob(self, *args):
        self.calls.append(("ttsx_frob", args))
        return self.rc

    def ttsx_frob_workspace_bytes(self, *args):
        self.calls.append(("ttsx_frob_workspace_bytes", args))
        return self.nbytes

    def ttsx_last_hip_error(self, h):
        return HIP_TEXT.encode()

    def ttsx_destroy(self, h):
        pass


class Bare(E.Handle):
    PREFIX = "ttsx"


def bare(monkeypatch, **kw):
    monkeypatch.setattr(E, "_stream", lambda device: STREAM)
    h = object.__new__(Bare)
    h._h, h._lib, h.device, h._ws = H, Recorder(**kw), None, None
    return h


def test_what_reaches_the_c_function(monkeypatch):
    h = bare(monkeypatch)
    a, b, tail = torch.zeros(3), torch.zeros(2, dtype=torch.int32), torch.zeros(1)
    ws = torch.empty(640, dtype=torch.uint8)
    arr = (C.c_void_p * 2)()
    h.call("ttsx_frob", a, None, 7, 0.5, True, arr, b, E.WS(ws), E.WS(None), E.STREAM, tail)
    (name, got), = h._lib.calls
    assert name == "ttsx_frob"
    want = (H, a.data_ptr(), None, 7, 0.5, True, arr, b.data_ptr(), ws.data_ptr(), 640, None, 0, STREAM, tail.data_ptr())
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert type(g) is type(w) and (g is w if w is arr else g == w), (i, g, w)


def test_a_refusal_raises_with_the_code_and_the_name(monkeypatch):
    h = bare(monkeypatch, rc=_lib.ERR_INVALID_ARG)
    with pytest.raises(_lib.TtsdecError) as e:
        h.call("ttsx_frob", 1, E.STREAM)
    assert e.value.code == _lib.ERR_INVALID_ARG and str(e.value).startswith("ttsx_frob: ") and HIP_TEXT not in str(e.value)
    assert not isinstance(e.value, _lib.DimsNotBuilt)

    h = bare(monkeypatch, rc=_lib.ERR_HIP)
    with pytest.raises(_lib.TtsdecError) as e:
        h.call("ttsx_frob")
    assert e.value.code == _lib.ERR_HIP and str(e.value).startswith("ttsx_frob: ") and f"[{HIP_TEXT}]" in str(e.value)


def test_err_dims_becomes_dims_not_built_where_a_message_is_given(monkeypatch):
    h = bare(monkeypatch, rc=_lib.ERR_DIMS)
    with pytest.raises(_lib.DimsNotBuilt) as e:
        h.call("ttsx_frob", 1, dims="B = 1: needs more")
    assert e.value.code == _lib.ERR_DIMS and str(e.value).startswith("ttsx_frob: ") and "[B = 1: needs more]" in str(e.value)
    with pytest.raises(_lib.TtsdecError) as e:
        h.call("ttsx_frob", 1)
    assert e.value.code == _lib.ERR_DIMS and not isinstance(e.value, _lib.DimsNotBuilt)
    h._lib.rc = _lib.OK
    h.call("ttsx_frob", 1, dims="B = 1: needs more")  # (the message alone raises nothing)


def test_the_sized_workspace_goes_through_workspace(monkeypatch):
    h = bare(monkeypatch, nbytes=1000)
    asked = []
    held = Bare.workspace
    monkeypatch.setattr(Bare, "workspace", lambda self, kind, nbytes: asked.append((kind, nbytes)) or held(self, kind, nbytes))
    ws = h.sized_workspace("frob", "ttsx_frob_workspace_bytes", 2, 30, refusal=ValueError("never"))
    assert h._lib.calls == [("ttsx_frob_workspace_bytes", (H, 2, 30))] and asked == [("frob", 1000)]
    assert ws.dtype == torch.uint8 and ws.numel() >= 1000 and h._ws["frob"] is ws
    h._lib.nbytes = 400
    assert h.sized_workspace("frob", "ttsx_frob_workspace_bytes", 1, 30) is ws and asked[-1] == ("frob", 400)  # grow-only

    h._lib.nbytes = 0
    refusal = _lib.DimsNotBuilt(_lib.ERR_DIMS, "ttsx_frob", "B = 70000: too many")
    with pytest.raises(_lib.DimsNotBuilt) as e:
        h.sized_workspace("frob", "ttsx_frob_workspace_bytes", 70000, 30, refusal=refusal)
    assert e.value is refusal and len(asked) == 2
    with pytest.raises(NotImplementedError, match="its own text"):
        h.sized_workspace("frob", "ttsx_frob_workspace_bytes", 70000, 30, refusal=NotImplementedError("its own text"))
