"""CPU: cancelling a request of a decode session, without a GPU (include/vc_engine.h vc_session_cancel): the symbol is exported and
bound with the header's three parameters and refuses a NULL engine, the Python surface is there, and session_cancel_k is in the compiled
gfx950 code with no scratch memory and no chain of waiting stores."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_store_scan as isa  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from voicecraft_amd import _lib
    return _lib.load()


def test_cancel_is_exported_bound_and_refuses_a_null_engine(lib):
    from voicecraft_amd import _lib
    assert hasattr(lib, "vc_session_cancel")
    res, args = _lib.PROTOTYPES["vc_session_cancel"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    header = open(os.path.join(ROOT, "include", "vc_engine.h")).read()
    m = re.search(r"^int vc_session_cancel\(([^)]*)\);", header, re.M)
    assert m, "vc_session_cancel is not declared in include/vc_engine.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(args) == 3, params
    assert params[0].startswith("vc_engine*") and params[1].startswith("int ") and params[2].startswith("int*"), params
    was = C.c_int(7)
    assert lib.vc_session_cancel(None, 1, C.byref(was)) == -1 and was.value == 7
    assert lib.vc_session_cancel(None, 1, None) == -1


def test_python_surface_has_cancel():
    from voicecraft_amd import DecodeSession, SessionStreamer
    assert callable(DecodeSession.cancel) and callable(SessionStreamer.cancel)


@pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
def test_session_cancel_k_is_compiled_for_gfx950_without_scratch(tmp_path):
    """session_cancel_k: present once, no scratch, at most one store that waits for an earlier one (the rule of tests/test_isa.py:
    every load is issued before the first store)."""
    src = os.path.join(ROOT, "voicecraft_amd", "csrc", "vc_tokens.hip")
    dst = str(tmp_path / "vc_tokens.s")
    r = subprocess.run([isa.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", src, "-o", dst],
                       cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kern = {isa.demangle(n).replace("void ", ""): v for n, v in isa.kernels(open(dst).read()).items()}
    sel = {n: v for n, v in kern.items() if n.startswith("session_cancel_k(")}
    assert len(sel) == 1, sorted(kern)
    (name, (body, scratch, vgpr)), = sel.items()
    assert scratch == 0, (name, scratch)
    chains, stores = isa.store_chains(body)
    assert stores >= 1 and chains <= 1, (name, chains, stores)
