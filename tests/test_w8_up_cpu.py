"""Option `w8u` without a GPU: the FFN up-projection on the 8-bit grid (quant.quantize_state_dict_w8(..., ffn_up=True): the image
bf16(linear1.weight * norm2.weight)), the pair planes of its 16-channel image W1 through the host export of the packer
(vc_w8w_pack_host) against quant.w8w_decode, the plan (vc_debug_w8u_plan: plan_pass itself with W1 taken as packed) for EVERY model
width the engine accepts, rows 1..64 and masks 0 / 2 / 10, and the new symbols.  vc_debug_w8w_plan must report what it reported."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from voicecraft_amd import _lib, quant, synth
from test_w8_wide_cpu import OFF_GRID, WIDTHS, cfg, image16, image_plan, pack_host, w8w_plan

MASKS = (0, 2, 10)
# the row counts at which the form is taken without bit 8 where it exists (csrc/vc_engine_host.h W8_FORMS, row `w8u`, from profiles/w8_up_ab.log)
ROWS_FFN_UP = range(17, 65)
KPW = {512: 2, 1024: 4, 2048: 8}                  # K = d over eight waves, in k-tiles of 32 inputs


def test_abi_new_symbols():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vc_engine.h")).read()
    for name in ("vc_request_w8_up", "vc_debug_w8u_plan"):
        fn = getattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert fn.restype is res and list(fn.argtypes) == args
        assert f"int {name}(" in header


# ------------------------------------------------------------------ the quantiser
@pytest.fixture(scope="module")
def model():
    a = synth.make_args("tiny128", num_decoder_layers=2)
    return a, synth.make_state_dict(a, seed=0, fast=True)


def test_quantiser_puts_the_folded_ffn_up_image_on_the_grid(model):
    a, sd = model
    before = {k: v.clone() for k, v in sd.items() if torch.is_tensor(v)}
    two = quant.quantize_state_dict_w8(a, sd)
    three = quant.quantize_state_dict_w8(a, sd, ffn_up=True)
    assert all(torch.equal(sd[k], before[k]) for k in before)                      # the input is not modified
    changed = sorted(k for k in before if not torch.equal(three[k], two[k]))
    assert changed == [f"decoder.layers.{l}.linear1.weight" for l in range(2)], changed
    for l in range(2):
        p = f"decoder.layers.{l}."
        img = quant.fold(three[p + "linear1.weight"], three[p + "norm2.weight"])
        assert torch.equal(quant.quantize_image(img), img)                           # the image is on the grid ...
        raw = quant.fold(sd[p + "linear1.weight"], sd[p + "norm2.weight"])
        assert torch.equal(img, quant.quantize_image(raw)) and not torch.equal(img, raw)      # ... the nearest grid point of the original's
        assert three[p + "linear1.weight"].dtype == torch.float32
        # every pair of the 16-channel image packs, and decodes to the image
        pairs = image16(img.numpy())
        assert pairs.shape[0] == (4 * a.d_model // 16) * (a.d_model // 64)
        planes, side, refused = pack_host(pairs)
        assert refused == 0
        assert np.array_equal(quant.w8w_decode(planes, side).numpy().view(np.uint32), pairs.view(np.uint32))
    again = quant.quantize_state_dict_w8(a, three, ffn_up=True)
    assert all(torch.equal(again[k], three[k]) for k in three if torch.is_tensor(three[k]))      # idempotent


def test_quantiser_default_is_what_it_was(model):
    a, sd = model
    got = quant.quantize_state_dict_w8(a, sd)
    assert sorted(got) == sorted(sd)
    for l in range(2):
        p = f"decoder.layers.{l}."
        want = {p + "linear2.weight": quant.quantize_matrix(sd[p + "linear2.weight"]),
                p + "self_attn.in_proj_weight": quant.quantize_matrix(sd[p + "self_attn.in_proj_weight"], sd[p + "norm1.weight"])}
        for k, v in want.items():
            assert torch.equal(got[k], v), k
    untouched = [k for k in sd if torch.is_tensor(sd[k]) and not (k.endswith("linear2.weight") or k.endswith("in_proj_weight"))]
    assert any(k.endswith("linear1.weight") for k in untouched)
    assert all(torch.equal(got[k], sd[k]) for k in untouched)
    assert all(torch.equal(quant.quantize_state_dict_w8(a, sd, ffn_up=False)[k], got[k]) for k in untouched + list(want))
    assert sorted(quant.MATRICES) == ["ffn_down", "qkv"]
    with pytest.raises(AssertionError):                                              # the third matrix is no name of `matrices`
        quant.quantize_state_dict_w8(a, sd, matrices=("ffn_up",))


def test_packer_refuses_exactly_the_pair_with_an_off_grid_value(model):
    a, sd = model
    d = a.d_model
    assert d == 512
    q = quant.quantize_state_dict_w8(a, sd, ffn_up=True)
    img = quant.fold(q["decoder.layers.1.linear1.weight"], q["decoder.layers.1.norm2.weight"]).clone()
    img[16 * 37 + 9, 64 * 5 + 40] = OFF_GRID         # tile 37, channel 9, inputs 320..383: pair 37 * (d / 64) + 5
    pairs = image16(img.numpy())
    planes, side, refused = pack_host(pairs)
    assert refused == 1
    back = quant.w8w_decode(planes, side).numpy()
    wrong = [p for p in range(pairs.shape[0]) if not np.array_equal(back[p], pairs[p])]
    assert wrong == [37 * (d // 64) + 5], wrong


# ------------------------------------------------------------------ the plan
def w8u_plan(d, h, mask, rows):
    c = cfg(d, h)
    out = (C.c_int32 * 2)()
    assert _lib.load().vc_debug_w8u_plan(C.byref(c), mask, rows, out) == 0
    return list(out)


@pytest.mark.parametrize("d,h", WIDTHS)
def test_w8u_plan_every_width(d, h):
    for rows in range(1, 65):
        img = image_plan(d, h, rows)
        # include/vc_engine.h vc_debug_plan: [1] form (2 = wide), [11] the layer runs on rows_gemm_wd_k, [14] k-tiles per wave for K = d
        wide = rows > 16 and img[1] == 2 and img[11] == 1
        kpw = img[14] if wide else 0
        may = wide and kpw in (2, 4, 8)
        for mask in MASKS:
            took, k = w8u_plan(d, h, mask, rows)
            want = bool(may and (mask & 2) and ((mask & 8) or rows in ROWS_FFN_UP))
            assert took == int(want) and k == (kpw if want else 0), (d, rows, mask, took, k)
            if rows <= 16 or mask == 0:
                assert [took, k] == [0, 0]


def test_w8u_plan_widths_with_a_form():
    for rows in (17, 32, 33, 64):
        by_d = {d: w8u_plan(d, h, 10, rows) for d, h in WIDTHS}
        assert {d: v[1] for d, v in by_d.items() if v[0]} == KPW, (rows, by_d)
    # without bit 8: exactly the rows of the committed table
    for d, h in WIDTHS:
        if d in KPW:
            assert [r for r in range(1, 65) if w8u_plan(d, h, 2, r)[0]] == list(ROWS_FFN_UP), d


def test_w8u_plan_bad_arguments():
    lib = _lib.load()
    c = cfg(2048, 16)
    out = (C.c_int32 * 2)()
    for rows in (0, -3, 65):
        assert lib.vc_debug_w8u_plan(C.byref(c), 2, rows, out) == -1
    for mask in (1, 3, 4, 5, 8, 13, 16, 18, -1):
        assert lib.vc_debug_w8u_plan(C.byref(c), mask, 33, out) == -1
    assert lib.vc_debug_w8u_plan(None, 2, 33, out) == -1
    assert lib.vc_debug_w8u_plan(C.byref(c), 2, 33, None) == -1


@pytest.mark.parametrize("d,h", WIDTHS)
def test_w8w_plan_reports_what_it_reported(d, h):
    """FFN-down and QKV: taken at every wide row count where the wave's K share is 2, 4 or 8 k-tiles (tests/test_w8_wide_cpu.py);
    bit 2 stays no bit of that option."""
    lib = _lib.load()
    out = (C.c_int32 * 4)()
    for rows in (1, 16, 17, 32, 33, 64):
        img = image_plan(d, h, rows)
        wide = rows > 16 and img[1] == 2 and img[11] == 1
        kpw_qkv = img[14] if wide else 0
        kpw_ffn = 4 * d // (32 * 8 * img[13]) if wide and img[13] > 0 and 4 * d % (32 * 8 * img[13]) == 0 else 0
        for mask in (0, 1, 4, 5, 9, 12, 13):
            ffn = int(bool(wide and (mask & 1) and kpw_ffn in (2, 4, 8)))
            qkv = int(bool(wide and (mask & 4) and kpw_qkv in (2, 4, 8)))
            assert w8w_plan(d, h, mask, rows) == [ffn, qkv, kpw_ffn if ffn else 0, kpw_qkv if qkv else 0], (d, rows, mask)
        for mask in (2, 7, 10, 15):
            assert lib.vc_debug_w8w_plan(C.byref(cfg(d, h)), mask, rows, out) == -1


# ------------------------------------------------------------------ the order of the requests (no device state is touched)
def test_request_order_python():
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args("tiny128", num_decoder_layers=1)
    with pytest.raises(ValueError, match="w8_up=True"):
        VoiceCraftEngine(a, {}, w8_up=True)
    assert VoiceCraftEngine.W8_UP_MASK == 2 and VoiceCraftEngine.LAUNCH_FORMS[-1] == "w8_up"
