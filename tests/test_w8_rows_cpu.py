"""Option `w8r` without a GPU (vc_debug_w8r_plan): which steps of 2..8 finished rows stream the FFN down-projection and the QKV
projection of layers 1.. as E4M3 bytes, for EVERY model width the engine accepts, rows 1..16 and every mask.  The function goes
through plan_pass itself with all matrices taken as packed, so what it reports is what the launch sites follow.  A w8 form may be
reported only where the image form it replaces is planned (vc_debug_plan: fr_pair / qkv_p8 = 2), the mask has the matrix's bit and a
wave's fragments per tile are whole groups of four; where it is reported the groups per wave are the launcher's."""
import ctypes as C

import pytest

from voicecraft_amd import _lib
from voicecraft_amd._lib import ModelCfg

WIDTHS = [(d, h) for d in range(256, 2049, 256) for h in (d // 32, d // 64, d // 128) if h >= 1 and d % h == 0 and d // h in (32, 64, 128)]
MASKS = (0, 1, 4, 5)
# the row counts at which the forms are taken where they exist (csrc/vc_engine_host.h W8_FORMS, row `w8r`, from profiles/w8_rows_ab.log)
ROWS_FFN_DOWN = range(2, 9)
ROWS_QKV = range(2, 7)       # rows_gemm_qp_k itself stops at 6 rows at d = 2048


def cfg(d, h):
    P, av = 1024, 2048
    return ModelCfg(d_model=d, nhead=h, num_layers=2, n_codebooks=4, audio_vocab_size=av, n_special=4, text_rows=101, head_hidden=P,
                    empty_token=av, eog=av + 1, audio_pad_token=av + 2, eos=av + 3, reduced_eog=1, encodec_sr=50, max_n_spans=3,
                    max_seqs=64, max_positions=1024)


def w8r_plan(d, h, mask, rows):
    c = cfg(d, h)
    out = (C.c_int32 * 4)()
    assert _lib.load().vc_debug_w8r_plan(C.byref(c), mask, rows, out) == 0
    return list(out)


def image_plan(d, h, rows):
    c = cfg(d, h)
    out = (C.c_int32 * 16)()
    assert _lib.load().vc_debug_plan(C.byref(c), _lib.VC_DTYPE_BF16, rows, out) == 0
    return list(out)


def test_abi_new_symbols():
    lib = _lib.load()
    for name in ("vc_request_w8_rows", "vc_debug_w8r_plan"):
        fn = getattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert fn.restype is res and list(fn.argtypes) == args


@pytest.mark.parametrize("d,h", WIDTHS)
def test_w8r_plan_every_width(d, h):
    for rows in range(1, 17):
        img = image_plan(d, h, rows)
        fr_form, qkv_p8, fr_pair = img[1], img[9], img[10]
        for mask in MASKS:
            ffn, qkv, ng_ffn, ng_qkv = w8r_plan(d, h, mask, rows)
            assert ffn in (0, 1) and qkv in (0, 1)
            # fragments per wave of a tile: K / 64 over eight waves
            npw_ffn, npw_qkv = 4 * d // 64 // 8, d // 64 // 8
            may_ffn = fr_form == 1 and fr_pair == 1 and (mask & 1) and 4 * d % 512 == 0 and npw_ffn % 4 == 0 and 2 <= rows <= 8
            may_qkv = fr_form == 1 and qkv_p8 == 2 and (mask & 4) and d % 512 == 0 and npw_qkv % 4 == 0 and 2 <= rows <= 8
            if ffn:
                assert may_ffn, (d, rows, mask)
                assert ng_ffn == 4 * d // 2048 and ng_ffn in (1, 2, 4)
            else:
                assert ng_ffn == 0
            if qkv:
                assert may_qkv, (d, rows, mask)
                assert d == 2048 and ng_qkv == 1
            else:
                assert ng_qkv == 0
            # ... and it IS taken at the row counts the measurement left it
            assert bool(ffn) == bool(may_ffn and rows in ROWS_FFN_DOWN), (d, rows, mask)
            assert bool(qkv) == bool(may_qkv and rows in ROWS_QKV), (d, rows, mask)
            if rows == 1 or rows > 8:
                assert [ffn, qkv, ng_ffn, ng_qkv] == [0, 0, 0, 0]


def test_w8r_plan_widths_with_a_form():
    """FFN-down: d = 512, 1024, 2048 with 1, 2, 4 groups per wave; QKV: d = 2048 alone (d = 1024 has half a group per wave and tile
    and stays on the image)."""
    got_ffn = {d: w8r_plan(d, h, 5, 3)[2] for d, h in WIDTHS}
    got_qkv = {d: w8r_plan(d, h, 5, 3)[3] for d, h in WIDTHS}
    assert {d: g for d, g in got_ffn.items() if g} == {512: 1, 1024: 2, 2048: 4}
    assert {d: g for d, g in got_qkv.items() if g} == {2048: 1}


def test_w8r_plan_bad_arguments():
    lib = _lib.load()
    c = cfg(2048, 16)
    out = (C.c_int32 * 4)()
    assert lib.vc_debug_w8r_plan(C.byref(c), 5, 0, out) == -1
    assert lib.vc_debug_w8r_plan(C.byref(c), 5, -3, out) == -1
    for mask in (2, 7, 8, -1):
        assert lib.vc_debug_w8r_plan(C.byref(c), mask, 3, out) == -1
    assert lib.vc_debug_w8r_plan(None, 5, 3, out) == -1
    assert lib.vc_debug_w8r_plan(C.byref(c), 5, 3, None) == -1
