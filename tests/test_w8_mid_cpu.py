"""Option `w8m` without a GPU (vc_debug_w8m_plan): which passes of 9..16 finished rows stream the FFN down-projection as E4M3 bytes, for
EVERY model width the engine accepts, rows 1..64 and every mask.  The function goes through plan_pass itself with the matrix taken as
packed, so what it reports is what the launch site follows.  The form may be reported only where the image launch it replaces is
planned (vc_debug_plan: finished rows, no paired producer, 9..16 rows) and the mask has bit 1; with bit 8 it is reported exactly where
a wave's k-tiles per piece are whole groups of eight in one chunk, without it exactly at the row counts the measurement left it.  The
neighbouring options `w8r` and `w8w` report what they reported."""
import ctypes as C

import pytest

from voicecraft_amd import _lib
from test_w8_rows_cpu import WIDTHS, cfg, image_plan, w8r_plan

MASKS = (0, 1, 8, 9)
# the row counts at which the form is taken without bit 8 where it exists (csrc/vc_engine_host.h W8_FORMS, row `w8m`, from profiles/w8_mid_ab.log)
ROWS_WIN = range(9, 17)      # measured at 9, 12 and 16 rows, every whole range below zero; the counts between follow the nearest
# d: (kernel: 1 = X in one piece, 2 = K in two halves; groups per wave and piece)
FORMS = {512: (1, 1), 1024: (1, 2), 2048: (2, 2)}


def w8m_plan(d, h, mask, rows):
    c = cfg(d, h)
    out = (C.c_int32 * 4)()
    assert _lib.load().vc_debug_w8m_plan(C.byref(c), mask, rows, out) == 0
    return list(out)


def w8w_plan(d, h, mask, rows):
    c = cfg(d, h)
    out = (C.c_int32 * 4)()
    assert _lib.load().vc_debug_w8w_plan(C.byref(c), mask, rows, out) == 0
    return list(out)


def test_abi_new_symbols():
    lib = _lib.load()
    for name in ("vc_request_w8_mid", "vc_debug_w8m_plan"):
        fn = getattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert fn.restype is res and list(fn.argtypes) == args


@pytest.mark.parametrize("d,h", WIDTHS)
def test_w8m_plan_every_width(d, h):
    for rows in range(1, 65):
        img = image_plan(d, h, rows)
        # include/vc_engine.h vc_debug_plan: [1] form (1 = finished rows), [5] the FFN-down producer's form, [10] the paired producer
        # (reported up to 8 rows only)
        image_launch = img[1] == 1 and img[10] != 1 and 9 <= rows <= 16
        for mask in MASKS:
            took, kernel, ng, zero = w8m_plan(d, h, mask, rows)
            assert took in (0, 1) and zero == 0
            may = bool(image_launch and (mask & 1) and d in FORMS)
            if took:
                assert may, (d, rows, mask)
                assert (kernel, ng) == FORMS[d], (d, rows, mask)
                assert kernel == img[5], (d, rows, mask)      # the twin of the kernel the image launch runs on
            else:
                assert (kernel, ng) == (0, 0)
            if mask & 8:
                assert bool(took) == may, (d, rows, mask)
            else:
                assert bool(took) == (may and rows in ROWS_WIN), (d, rows, mask)
            if rows <= 8 or rows >= 17:
                assert [took, kernel, ng, zero] == [0, 0, 0, 0]


def test_w8m_plan_widths_with_a_form():
    """d = 512 and 1024: X of 9..16 rows fits LDS in one piece, a wave owns 8 / 16 k-tiles = 1 / 2 groups; d = 2048: K in two halves,
    16 k-tiles = 2 groups per half; at every row count 9..16.  Every other width has a wave share that is no whole group in one chunk."""
    for rows in range(9, 17):
        got = {d: tuple(w8m_plan(d, h, 9, rows)[1:3]) for d, h in WIDTHS if w8m_plan(d, h, 9, rows)[0]}
        assert got == FORMS, (rows, got)
        assert {d for d, h in WIDTHS if w8m_plan(d, h, 1, rows)[0]} == (set(FORMS) if rows in ROWS_WIN else set()), rows


def test_w8m_plan_bad_arguments():
    lib = _lib.load()
    c = cfg(2048, 16)
    out = (C.c_int32 * 4)()
    assert lib.vc_debug_w8m_plan(C.byref(c), 1, 0, out) == -1
    for mask in (2, 4, 5, 16, -1):
        assert lib.vc_debug_w8m_plan(C.byref(c), mask, 12, out) == -1
    assert lib.vc_debug_w8m_plan(None, 1, 12, out) == -1
    assert lib.vc_debug_w8m_plan(C.byref(c), 1, 12, None) == -1


def test_neighbouring_plans_report_what_they_reported():
    """`w8r` stops at 8 rows, `w8w` starts at 17: the rows either side of the new range."""
    assert w8r_plan(2048, 16, 5, 8) == [1, 0, 4, 0]      # FFN-down on four groups per wave; QKV stops at 6 rows at d = 2048
    assert w8r_plan(2048, 16, 5, 6) == [1, 1, 4, 1]
    assert w8r_plan(2048, 16, 5, 9) == [0, 0, 0, 0]
    assert w8r_plan(1024, 16, 5, 8) == [1, 0, 2, 0]
    assert w8r_plan(1024, 16, 5, 9) == [0, 0, 0, 0]
    assert w8w_plan(2048, 16, 5, 16) == [0, 0, 0, 0]
    assert w8w_plan(2048, 16, 5, 17) == [1, 1, 8, 8]
    assert w8w_plan(1024, 16, 13, 16) == [0, 0, 0, 0]
    assert w8w_plan(1024, 16, 13, 17) == [1, 1, 4, 4]


def test_request_order_python():
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args("tiny128", num_decoder_layers=1)
    with pytest.raises(ValueError, match="w8_mid=True"):
        VoiceCraftEngine(a, {}, w8_mid=True)
    assert VoiceCraftEngine.W8_MID_MASK == 1
