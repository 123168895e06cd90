"""Option `w8ur` without a GPU: the plan (vc_debug_w8ur_plan: plan_pass itself with W1 taken as packed) for EVERY model width the
engine accepts, rows 1..64 and masks 0 / 2 / 10 against vc_debug_plan, the new symbols, the order of the requests, the compiled
kernels (nine rows_gemm_lnq_w8_k instantiations, no scratch, the E4M3 conversion in each) and the neighbouring plans, which must
report what they reported."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from voicecraft_amd import _lib, synth
from test_w8_mid_cpu import w8m_plan
from test_w8_up_cpu import w8u_plan
from test_w8_wide_cpu import ROOT, WIDTHS, cfg, image_plan, isa, w8w_plan      # (isa: tools/isa_store_scan.py)

MASKS = (0, 2, 10)
# the row counts at which the form is taken without bit 8 where it exists (csrc/vc_engine_host.h W8_FORMS, row `w8ur`, from profiles/w8_up_rows_ab.log)
ROWS_WIN = range(2, 17)
KTW = {512: 4, 1024: 8, 2048: 16}                 # K = d over the four waves of a tile, in k-tiles of 32 inputs, one chunk


def w8ur_plan(d, h, mask, rows):
    c = cfg(d, h)
    out = (C.c_int32 * 2)()
    assert _lib.load().vc_debug_w8ur_plan(C.byref(c), mask, rows, out) == 0
    return list(out)


def test_abi_new_symbols():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vc_engine.h")).read()
    for name in ("vc_request_w8_up_rows", "vc_debug_w8ur_plan"):
        fn = getattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert fn.restype is res and list(fn.argtypes) == args
        assert f"int {name}(" in header


@pytest.mark.parametrize("d,h", WIDTHS)
def test_w8ur_plan_every_width(d, h):
    for rows in range(1, 65):
        img = image_plan(d, h, rows)
        # include/vc_engine.h vc_debug_plan: [1] form (1 = finished rows).  The consumers read the centred copy (option hq, the default)
        # where a bf16 row is whole 1 KB requests of a wave: d a multiple of 512
        hq = d % 512 == 0 and 2 * d <= 8192
        may = img[1] == 1 and hq and d in KTW
        for mask in MASKS:
            took, k = w8ur_plan(d, h, mask, rows)
            want = bool(may and (mask & 2) and ((mask & 8) or rows in ROWS_WIN))
            assert took == int(want) and k == (KTW[d] if want else 0), (d, rows, mask, took, k)
            if rows == 1 or rows >= 17 or mask == 0:
                assert [took, k] == [0, 0]


def test_w8ur_plan_widths_with_a_form():
    """Every row count 2..16 is a finished-row pass at the three widths (vc_debug_plan), so bit 8 takes the form at all of them."""
    for rows in range(2, 17):
        by_d = {d: w8ur_plan(d, h, 10, rows) for d, h in WIDTHS}
        assert {d: v[1] for d, v in by_d.items() if v[0]} == KTW, (rows, by_d)
    # without bit 8: exactly the rows of the committed table
    for d, h in WIDTHS:
        if d in KTW:
            assert [r for r in range(1, 65) if w8ur_plan(d, h, 2, r)[0]] == list(ROWS_WIN), d


def test_w8ur_plan_bad_arguments():
    lib = _lib.load()
    c = cfg(2048, 16)
    out = (C.c_int32 * 2)()
    for rows in (0, -3, 65):
        assert lib.vc_debug_w8ur_plan(C.byref(c), 2, rows, out) == -1
    for mask in (1, 3, 4, 5, 8, 13, 16, 18, -1):
        assert lib.vc_debug_w8ur_plan(C.byref(c), mask, 8, out) == -1
    assert lib.vc_debug_w8ur_plan(None, 2, 8, out) == -1
    assert lib.vc_debug_w8ur_plan(C.byref(c), 2, 8, None) == -1


def test_neighbouring_plans_report_what_they_reported():
    """`w8u` starts at 17 rows, `w8w` too, `w8m` covers 9..16 with the FFN down-projection: none of them moved."""
    assert w8u_plan(2048, 16, 10, 16) == [0, 0] and w8u_plan(2048, 16, 2, 17) == [1, 8] and w8u_plan(512, 8, 10, 64) == [1, 2]
    assert w8u_plan(1024, 16, 2, 8) == [0, 0] and w8u_plan(1024, 16, 0, 33) == [0, 0] and w8u_plan(1024, 16, 2, 33) == [1, 4]
    assert w8w_plan(2048, 16, 5, 16) == [0, 0, 0, 0] and w8w_plan(2048, 16, 5, 17) == [1, 1, 8, 8]
    assert w8w_plan(1024, 16, 13, 17) == [1, 1, 4, 4]
    assert w8m_plan(2048, 16, 1, 8) == [0, 0, 0, 0] and w8m_plan(2048, 16, 1, 9) == [1, 2, 2, 0] and w8m_plan(2048, 16, 1, 17) == [0, 0, 0, 0]
    assert w8m_plan(512, 8, 9, 16) == [1, 1, 1, 0] and w8m_plan(1024, 16, 1, 12) == [1, 1, 2, 0]


# ------------------------------------------------------------------ the order of the requests
def test_request_order():
    """ValueError without `w8=`; the C request on a null handle; and on a bare handle where vc_create gives one (it selects a device and
    touches nothing else, so it needs one: tests/test_gpu_w8_up_rows.py repeats the walk where a GPU is certain)."""
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args("tiny128", num_decoder_layers=1)
    with pytest.raises(ValueError, match="w8_up_rows=True"):
        VoiceCraftEngine(a, {}, w8_up_rows=True)
    assert VoiceCraftEngine.W8_UP_ROWS_MASK == 2 and VoiceCraftEngine.LAUNCH_FORMS[-1] == "w8_up"
    assert VoiceCraftEngine.LAUNCH_FORMS_MORE == ("w8_up_rows",) and "w8_up_rows" not in VoiceCraftEngine.LAUNCH_FORMS
    lib = _lib.load()
    assert lib.vc_request_w8_up_rows(None, 2) == -1
    h = C.c_void_p()
    c_ = cfg(a.d_model, a.nhead)
    if lib.vc_create(C.byref(c_), 0, C.byref(h)) == 0:
        try:
            assert lib.vc_request_w8_up_rows(h, 2) == -2            # VC_ESTATE: after vc_request_w8 only
            assert lib.vc_request_w8(h, 1) == 0                     # (it needs the request, none of its bits)
            for bad in (0, 1, 4, 5, 7, 10, -1):
                assert lib.vc_request_w8_up_rows(h, bad) == -1      # VC_EINVAL
            assert lib.vc_request_w8_up_rows(h, 2) == 0
            assert lib.vc_request_w8_up(h, 2) == 0                  # the two requests do not exclude each other
        finally:
            lib.vc_destroy(h)


# ------------------------------------------------------------------ the compiled kernels
@pytest.mark.skipif(not (os.path.exists(isa.HIPCC) or shutil.which(isa.HIPCC)), reason="hipcc not available")
def test_isa_of_the_new_instantiations(tmp_path):
    src = os.path.join(ROOT, "voicecraft_amd", "csrc", "vc_gemm_w8.hip")
    dst = str(tmp_path / "vc_gemm_w8.s")
    r = subprocess.run([isa.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", src, "-o", dst],
                       cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for name, (body, private_segment, vgpr) in isa.kernels(open(dst).read()).items():      # (.amdhsa_private_segment_fixed_size, .amdhsa_next_free_vgpr)
        m = re.search(r"rows_gemm_lnq_w8_k<(\d+), (\d+), (true|false)>", isa.demangle(name))
        if not m:
            continue
        seen.add((int(m.group(1)), int(m.group(2)), m.group(3) == "true"))
        assert private_segment == 0, (name, private_segment)
        assert vgpr <= 256, (name, vgpr)
        assert "v_cvt_scalef32_pk_bf16_fp8" in body, name
    assert seen == {(k, n, r2) for k in (4, 8, 16) for n, r2 in ((1, False), (2, False), (2, True))}, seen
