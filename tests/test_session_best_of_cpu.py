"""CPU: the boundary of best-of-N requests in a decode session (include/vc_engine.h vc_session_open_best_of,
vc_session_submit_best_of, vc_session_kept) without a GPU: the symbols are exported, bound with the header's parameter counts and refuse
null or invalid arguments without touching a device; the Python surface is as documented; the session's sampler pair, its FIRST forms and
the group table kernel are in the compiled gfx950 code and use no scratch."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_store_scan as isa  # noqa: E402

NEW = {"vc_session_open_best_of": 5, "vc_session_submit_best_of": 9, "vc_session_kept": 3}


@pytest.fixture(scope="module")
def lib():
    from voicecraft_amd import _lib
    return _lib.load()


def test_new_symbols_are_exported_and_bound_with_the_headers_parameter_counts(lib):
    from voicecraft_amd import _lib
    src = open(os.path.join(ROOT, "include", "vc_engine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_par in NEW.items():
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES and _lib.PROTOTYPES[name][0] is C.c_int, name
        assert len(_lib.PROTOTYPES[name][1]) == n_par, (name, len(_lib.PROTOTYPES[name][1]))
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/vc_engine.h"
        assert len(m.group(1).split(",")) == n_par, (name, m.group(1))
    # vc_session_fetch and vc_session_stats keep their signatures
    assert len(_lib.PROTOTYPES["vc_session_fetch"][1]) == 6 and len(_lib.PROTOTYPES["vc_session_stats"][1]) == 2


def test_new_entry_points_refuse_null_and_invalid_arguments_without_a_device(lib):
    from voicecraft_amd import _lib
    t, k = C.c_int(0), C.c_int(0)
    sc = _lib.SampleCfg()
    ctl = _lib.RequestCtl(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=-1)
    assert lib.vc_session_open_best_of(None, 4, 3, C.byref(sc), None) == -1
    assert lib.vc_session_open_best_of(None, 4, 0, None, None) == -1
    assert lib.vc_session_submit_best_of(None, None, 1, None, 0, 3, C.byref(ctl), 0, C.byref(t)) == -1
    assert lib.vc_session_submit_best_of(None, None, 1, None, 0, 0, None, 0, None) == -1
    assert lib.vc_session_kept(None, 1, C.byref(k)) == -1
    assert lib.vc_session_kept(None, 1, None) == -1


def test_python_surface():
    from voicecraft_amd import DecodeSession, inference_tts_queue
    from voicecraft_amd.engine import VoiceCraftEngine
    p = inspect.signature(VoiceCraftEngine.open_session).parameters
    assert "max_samples" in p and p["max_samples"].default == 1
    p = inspect.signature(DecodeSession.submit).parameters
    assert "n_samples" in p and p["n_samples"].default == 1
    assert "n_samples" not in inspect.signature(DecodeSession.submit_edit).parameters     # the reference has no best-of-N editing
    for f in (VoiceCraftEngine.inference_tts_queue, inference_tts_queue):
        assert "batch_size" in inspect.signature(f).parameters, f
    assert inspect.signature(VoiceCraftEngine.inference_tts_queue).parameters["batch_size"].default == 1


def test_record_word_6_is_free_for_kept_and_the_record_keeps_its_size():
    h = open(os.path.join(ROOT, "voicecraft_amd", "csrc", "vc_common.h")).read()
    assert re.search(r"#define VC_SESS_REC_SPANS 8\b", h)
    tok = open(os.path.join(ROOT, "voicecraft_amd", "csrc", "vc_tokens.hip")).read()
    used = sorted({int(i) for i in re.findall(r"__hip_atomic_store\(rec \+ (\d)\b", tok)})
    assert used == [0, 1, 2, 3, 5, 6], used               # ([4] is written at admission by session_turn_k)


def _kernels(unit, tmp_path):
    src = os.path.join(ROOT, "voicecraft_amd", "csrc", unit + ".hip")
    dst = str(tmp_path / (unit + ".s"))
    r = subprocess.run([isa.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", src, "-o", dst],
                       cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return {isa.demangle(n).replace("void ", ""): v for n, v in isa.kernels(open(dst).read()).items()}


@pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
def test_the_new_kernels_are_compiled_for_gfx950_without_scratch(tmp_path):
    kern = _kernels("vc_tokens", tmp_path)
    for prefix in ("session_sample_only_k(", "session_first_sample_only_k(", "session_advance_only_k(",
                   "session_first_advance_only_k(", "session_groups_k("):
        sel = {n: v for n, v in kern.items() if n.startswith(prefix)}
        assert len(sel) == 1, (prefix, sorted(kern))
        for name, (body, scratch, vgpr) in sel.items():
            assert scratch == 0 and "scratch_" not in body, (name, scratch)
    # ... next to the kernels of a session opened without max_samples, which are still there under their names
    for prefix in ("sample_session_k<true>(", "sample_session_k<false>(", "session_turn_k("):
        assert sum(n.startswith(prefix) for n in kern) == 1, prefix
