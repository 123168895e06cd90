"""The six w8 plans side by side, without a GPU: vc_debug_w8r_plan, vc_debug_w8m_plan, vc_debug_w8w_plan, vc_debug_w8u_plan,
vc_debug_w8ur_plan and vc_debug_w8q_plan (plan_pass itself, every matrix taken as packed) for EVERY model width the engine accepts,
every row count 0..65 and every mask -1..16, against one statement of the rule per form.  The statement is built from FORMS below,
which mirrors what include/vc_engine.h says of each option: the legal values, the matrix behind each bit, the image launch the
form replaces (read off vc_debug_plan), the row counts the measured table takes, and whether bit 8 ("every row count") exists.  The
per-option files (tests/test_w8_*_cpu.py) state the same rules one by one and walk a handful of bad masks each."""
import ctypes as C

import pytest

from voicecraft_amd import _lib
from test_w8_rows_cpu import WIDTHS, cfg

ROWS = range(0, 66)
MASKS = range(-1, 17)
D3 = (512, 1024, 2048)            # the widths at which a wave's share of every matrix is whole groups / pairs


def hq(d):      # the consumers read the centred copy (option hq, the default): a bf16 row is whole 1 KB requests of a wave
    return d % 512 == 0 and 2 * d <= 8192


def wide(img):      # vc_debug_plan: [1] = 2 wide step, [11] the layer runs on rows_gemm_wd_k
    return img[1] == 2 and img[11] == 1


def kpw_f2(d, img):      # k-tiles per wave of an FFN-down slice: K = 4 d over [13] slices and eight waves
    return 4 * d // (32 * 8 * img[13]) if img[13] > 0 and 4 * d % (32 * 8 * img[13]) == 0 else 0


# One entry per matrix of a form: (bit, out slot of "taken", the image launch is planned and the launcher has a form, rows the table
# takes, [(out slot, figure reported where taken), ..]).  d: model width, rows: row count, img: vc_debug_plan of (d, rows) in bf16.
FORMS = {
    # steps of 2..8 finished rows: FFN-down on the paired producer ([10]), QKV on the paired consumer ([9] = 2); no bit 8
    "w8r": dict(fn="vc_debug_w8r_plan", n_out=4, legal={0, 1, 4, 5}, bit8=False, matrices=[
        (1, 0, lambda d, rows, img: img[1] == 1 and rows <= 8 and img[10] == 1 and d in D3, range(2, 9), [(2, lambda d, img: d // 512)]),
        (4, 1, lambda d, rows, img: img[1] == 1 and rows <= 8 and img[9] == 2 and d == 2048, range(2, 9), [(3, lambda d, img: 1)])]),
    # passes of 9..16 finished rows: FFN-down on rows_gemm_fr_k ([5] = 1: d = 512 one group, 1024 two) / rows_gemm_fr2_k ([5] = 2: two)
    "w8m": dict(fn="vc_debug_w8m_plan", n_out=4, legal={0, 1, 8, 9}, bit8=True, matrices=[
        (1, 0, lambda d, rows, img: img[1] == 1 and 9 <= rows <= 16 and d in D3, range(9, 17),
         [(1, lambda d, img: img[5]), (2, lambda d, img: {512: 1, 1024: 2, 2048: 2}[d])])]),
    # steps of 17..64 rows on the staged wide kernel: FFN-down on its split-K slices, QKV on K = d ([14] k-tiles per wave)
    "w8w": dict(fn="vc_debug_w8w_plan", n_out=4, legal={0, 1, 4, 5, 8, 9, 12, 13}, bit8=True, matrices=[
        (1, 0, lambda d, rows, img: wide(img) and kpw_f2(d, img) in (2, 4, 8), range(17, 65), [(2, kpw_f2)]),
        (4, 1, lambda d, rows, img: wide(img) and img[14] in (2, 4, 8), range(17, 65), [(3, lambda d, img: img[14])])]),
    # ... and FFN-up there (K = d)
    "w8u": dict(fn="vc_debug_w8u_plan", n_out=2, legal={0, 2, 10}, bit8=True, matrices=[
        (2, 0, lambda d, rows, img: wide(img) and img[14] in (2, 4, 8), range(17, 65), [(1, lambda d, img: img[14])])]),
    # passes of 2..16 finished rows: FFN-up behind a centred copy, K = d over four waves in one chunk
    "w8ur": dict(fn="vc_debug_w8ur_plan", n_out=2, legal={0, 2, 10}, bit8=True, matrices=[
        (2, 0, lambda d, rows, img: img[1] == 1 and hq(d) and d in D3, range(2, 17), [(1, lambda d, img: d // 128)])]),
    # ... and QKV of layers 1.. where the paired consumer ([9] = 2) leaves the 12-channel image in place
    "w8q": dict(fn="vc_debug_w8q_plan", n_out=2, legal={0, 4, 12}, bit8=True, matrices=[
        (4, 0, lambda d, rows, img: img[1] == 1 and hq(d) and d in D3 and img[9] != 2, range(5, 17), [(1, lambda d, img: d // 128)])]),
}


def want(form, d, rows, mask, img):
    """(return code, out[]) of one call by the rule; out is None where the call is refused."""
    if not 1 <= rows <= 64 or mask not in form["legal"]:
        return -1, None
    out = [0] * form["n_out"]
    for bit, slot, may, win, figures in form["matrices"]:
        if (mask & bit) and may(d, rows, img) and (rows in win or (form["bit8"] and (mask & 8))):
            out[slot] = 1
            for at, figure in figures:
                out[at] = figure(d, img)
    return 0, out


@pytest.mark.parametrize("d,h", WIDTHS)
def test_every_form_every_rows_every_mask(d, h):
    lib = _lib.load()
    c = cfg(d, h)
    img16 = (C.c_int32 * 16)()
    for rows in ROWS:
        img = None
        if 1 <= rows <= 64:
            assert lib.vc_debug_plan(C.byref(c), _lib.VC_DTYPE_BF16, rows, img16) == 0
            img = list(img16)
        for name, form in FORMS.items():
            fn = getattr(lib, form["fn"])
            for mask in MASKS:
                out = (C.c_int32 * 4)(-7, -7, -7, -7)
                rc = fn(C.byref(c), mask, rows, out)
                rc_want, out_want = want(form, d, rows, mask, img)
                assert rc == rc_want, (name, d, rows, mask, rc)
                if rc == 0:
                    assert list(out)[:form["n_out"]] == out_want, (name, d, rows, mask, list(out), out_want)
                    assert list(out)[form["n_out"]:] == [-7] * (4 - form["n_out"]), (name, d, rows, mask)      # two-word plans write two words


def test_null_arguments():
    lib = _lib.load()
    c = cfg(2048, 16)
    out = (C.c_int32 * 4)()
    for name, form in FORMS.items():
        fn = getattr(lib, form["fn"])
        mask = max(form["legal"])
        assert fn(None, mask, 12, out) == -1 and fn(C.byref(c), mask, 12, None) == -1, name
        assert fn(C.byref(c), mask, 12, out) == 0, name
