"""Option `w8w` without a GPU: the pair planes of the 16-channel images that 17..64-row steps stream (csrc/vc_w8.h), through the host
export of the packer (vc_w8w_pack_host) against the layout as voicecraft_amd/quant.py w8w_decode restates it; the plan
(vc_debug_w8w_plan, plan_pass itself with every matrix taken as packed) for EVERY model width the engine accepts, rows 1..64 and every
mask; the order of the requests; and the compiled kernels (private segment 0, <= 256 VGPRs, the conversion instruction)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from voicecraft_amd import _lib, quant
from test_w8_rows_cpu import WIDTHS, cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_store_scan as isa  # noqa: E402

MASKS = (0, 1, 4, 5)
OFF_GRID = (1.0 + 2.0 ** -7) * 2.0 ** -6          # eight significant bits: on no E4M3 grid
# the row counts at which the forms are taken without bit 8 where they exist (csrc/vc_engine_host.h W8_FORMS, row `w8w`, from profiles/w8_wide_ab.log)
ROWS_FFN_DOWN = range(17, 65)
ROWS_QKV = range(17, 65)


def test_abi_new_symbols():
    lib = _lib.load()
    for name in ("vc_request_w8_wide", "vc_debug_w8w_plan", "vc_w8w_pack_host"):
        fn = getattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert fn.restype is res and list(fn.argtypes) == args


# ------------------------------------------------------------------ the packer
def image16(w):
    """pack_k's th = 16 layout of a bf16-valued fp32 matrix [N, K]: [tile, k-tile, lane, value], lane l = channel 16 nt + (l & 15),
    inputs 32 kt + 8 (l >> 4) .. + 7; as pairs [n_pairs, 2, 64, 8] (k-tiles 2j, 2j + 1 of one tile, tile major)."""
    n, k = w.shape
    assert n % 16 == 0 and k % 64 == 0
    lane = np.arange(64)
    img = np.empty((n // 16, k // 32, 64, 8), np.float32)
    for nt in range(n // 16):
        for kt in range(k // 32):
            rows = 16 * nt + (lane & 15)
            cols = 32 * kt + 8 * (lane >> 4)
            img[nt, kt] = w[rows[:, None], cols[:, None] + np.arange(8)[None, :]]
    return img.reshape(-1, 2, 64, 8)


def pack_host(pairs):
    """float32 pairs [n, 2, 64, 8] of bf16 values -> (planes uint8 [n, 1024], side uint8 [n, 2], refused pairs)"""
    bits = torch.from_numpy(np.ascontiguousarray(pairs)).bfloat16().view(torch.int16).contiguous()
    assert bool((bits.view(torch.bfloat16).float() == torch.from_numpy(np.ascontiguousarray(pairs))).all())
    n = pairs.shape[0]
    planes = torch.full((n, 1024), 0xAA, dtype=torch.uint8)
    side = torch.full((n, 2), 0xAA, dtype=torch.uint8)
    refused = C.c_int32(-1)
    rc = _lib.load().vc_w8w_pack_host(C.c_void_p(bits.data_ptr()), n, C.c_void_p(planes.data_ptr()), C.c_void_p(side.data_ptr()),
                                      C.byref(refused))
    assert rc == 0
    return planes, side, refused.value


@pytest.mark.parametrize("shape", [(64, 256), (48, 128)])
def test_packer_round_trip_on_quantised_matrices(shape):
    g = torch.Generator().manual_seed(5 + shape[0])
    # rows of very different magnitude, so that the blocks' shifts differ
    w = (torch.randn(shape, generator=g) * torch.logspace(-3, 1, shape[0])[:, None]).bfloat16().float()
    q = quant.quantize_image(w)
    pairs = image16(q.numpy())
    assert pairs.shape[0] == shape[0] // 16 * (shape[1] // 64)
    planes, side, refused = pack_host(pairs)
    assert refused == 0
    back = quant.w8w_decode(planes, side).numpy()
    assert back.shape == pairs.shape and np.array_equal(back.view(np.uint32), pairs.view(np.uint32))
    assert (side[:, 0] != side[:, 1]).any()          # the halves of a pair carry their own shifts
    # the side bytes are the quantiser's own blocks: channels 0..7 / 8..15 of the tile x the pair's 64 inputs
    amax = np.abs(pairs).transpose(0, 2, 1, 3).reshape(-1, 4, 2, 8, 16).max(axis=(1, 3, 4))      # [pair, half]: lanes = (kg, half, c)
    for p in range(pairs.shape[0]):
        for h in range(2):
            s = int(side[p, h]) - 127
            # the smallest shift that holds the block: its maximum in E4M3's top binade (256 .. 448), or 240 where 480 would be the NaN code
            assert amax[p, h] == 0 or 240.0 * 2.0 ** s <= amax[p, h] <= 448.0 * 2.0 ** s, (p, h, s, amax[p, h])


def test_packer_halves_two_to_the_six_apart():
    lane = np.arange(64)
    pair = np.zeros((1, 2, 64, 8), np.float32)
    pair[0, :, (lane & 8) == 0, :] = 1.5             # channels 0..7
    pair[0, :, (lane & 8) != 0, :] = 1.5 * 64.0      # channels 8..15
    planes, side, refused = pack_host(pair)
    assert refused == 0
    assert int(side[0, 1]) - int(side[0, 0]) == 6
    assert int(side[0, 0]) - 127 == 0 - 8            # 1.5 = 384 . 2^-8: the top binade
    assert np.array_equal(quant.w8w_decode(planes, side).numpy(), pair)
    assert len(set(planes[0].tolist())) == 1         # the same code everywhere: the magnitudes live in the side bytes


def test_packer_refuses_exactly_the_pair_with_an_off_grid_value():
    w = quant.quantize_image(torch.randn(32, 256, generator=torch.Generator().manual_seed(3)).bfloat16().float())
    w[16 + 11, 70] = OFF_GRID                        # tile 1, channel 11, inputs 64..127: pair 1 * 4 + 1
    assert float(torch.tensor(OFF_GRID).bfloat16()) == OFF_GRID
    pairs = image16(w.numpy())
    planes, side, refused = pack_host(pairs)
    assert refused == 1
    back = quant.w8w_decode(planes, side).numpy()
    wrong = [p for p in range(pairs.shape[0]) if not np.array_equal(back[p], pairs[p])]
    assert wrong == [5], wrong
    for p in range(pairs.shape[0]):                  # ... and pair by pair: only that one is refused
        assert pack_host(pairs[p:p + 1])[2] == (1 if p == 5 else 0), p


def test_packer_pair_of_zeros_takes_shift_zero():
    planes, side, refused = pack_host(np.zeros((2, 2, 64, 8), np.float32))
    assert refused == 0 and side.tolist() == [[127, 127], [127, 127]] and int(planes.max()) == 0
    neg = np.zeros((1, 2, 64, 8), np.float32)
    neg[0, 1, 9, 3] = -0.0
    planes, side, refused = pack_host(neg)
    assert refused == 0 and side.tolist() == [[127, 127]]
    assert np.array_equal(quant.w8w_decode(planes, side).numpy().view(np.uint32), neg.view(np.uint32))


def test_packer_bad_arguments():
    lib = _lib.load()
    buf = (C.c_uint8 * 2048)()
    r = C.c_int32(0)
    assert lib.vc_w8w_pack_host(None, 1, buf, buf, C.byref(r)) == -1
    assert lib.vc_w8w_pack_host(buf, 1, None, buf, C.byref(r)) == -1
    assert lib.vc_w8w_pack_host(buf, 1, buf, None, C.byref(r)) == -1
    assert lib.vc_w8w_pack_host(buf, 1, buf, buf, None) == -1
    assert lib.vc_w8w_pack_host(buf, -1, buf, buf, C.byref(r)) == -1


# ------------------------------------------------------------------ the plan
def w8w_plan(d, h, mask, rows):
    c = cfg(d, h)
    out = (C.c_int32 * 4)()
    assert _lib.load().vc_debug_w8w_plan(C.byref(c), mask, rows, out) == 0
    return list(out)


def image_plan(d, h, rows):
    c = cfg(d, h)
    out = (C.c_int32 * 16)()
    assert _lib.load().vc_debug_plan(C.byref(c), _lib.VC_DTYPE_BF16, rows, out) == 0
    return list(out)


@pytest.mark.parametrize("d,h", WIDTHS)
def test_w8w_plan_every_width(d, h):
    for rows in range(1, 65):
        img = image_plan(d, h, rows)
        # include/vc_engine.h vc_debug_plan: [1] form (2 = wide), [11] the layer runs on rows_gemm_wd_k, [13] K slices of FFN-down,
        # [14] k-tiles per wave for K = d; the staged form is the default (option wd_stage = 1) and needs >= 2 k-tiles per wave
        wide = rows > 16 and img[1] == 2 and img[11] == 1
        kpw_qkv = img[14] if wide else 0
        kpw_ffn = 4 * d // (32 * 8 * img[13]) if wide and img[13] > 0 and 4 * d % (32 * 8 * img[13]) == 0 else 0
        for base in MASKS:
            for mask in (base, base | 8):
                ffn, qkv, k_ffn, k_qkv = w8w_plan(d, h, mask, rows)
                assert ffn in (0, 1) and qkv in (0, 1)
                may_ffn = bool(wide and (mask & 1) and kpw_ffn in (2, 4, 8))
                may_qkv = bool(wide and (mask & 4) and kpw_qkv in (2, 4, 8))
                if mask & 8:
                    assert bool(ffn) == may_ffn and bool(qkv) == may_qkv, (d, rows, mask)
                else:
                    assert bool(ffn) == (may_ffn and rows in ROWS_FFN_DOWN), (d, rows, mask)
                    assert bool(qkv) == (may_qkv and rows in ROWS_QKV), (d, rows, mask)
                assert k_ffn == (kpw_ffn if ffn else 0) and k_qkv == (kpw_qkv if qkv else 0), (d, rows, mask)
                if rows <= 16:
                    assert [ffn, qkv, k_ffn, k_qkv] == [0, 0, 0, 0]


def test_w8w_plan_widths_with_a_form():
    """QKV: K = d over eight waves is 2, 4, 8 k-tiles at d = 512, 1024, 2048.  FFN-down runs on four split-K slices of K = 4 d there:
    the same k-tiles per wave.  Every other width has a wave share the wide kernel has no form for, or one k-tile (d = 256)."""
    by_d = {d: w8w_plan(d, h, 13, 40) for d, h in WIDTHS}
    assert {d: v[3] for d, v in by_d.items() if v[1]} == {512: 2, 1024: 4, 2048: 8}
    assert {d: v[2] for d, v in by_d.items() if v[0]} == {512: 2, 1024: 4, 2048: 8}


def test_w8w_plan_bad_arguments():
    lib = _lib.load()
    c = cfg(2048, 16)
    out = (C.c_int32 * 4)()
    assert lib.vc_debug_w8w_plan(C.byref(c), 5, 0, out) == -1
    assert lib.vc_debug_w8w_plan(C.byref(c), 5, -3, out) == -1
    assert lib.vc_debug_w8w_plan(C.byref(c), 5, 65, out) == -1
    for mask in (2, 7, 16, 21, -1):
        assert lib.vc_debug_w8w_plan(C.byref(c), mask, 33, out) == -1
    assert lib.vc_debug_w8w_plan(None, 5, 33, out) == -1
    assert lib.vc_debug_w8w_plan(C.byref(c), 5, 33, None) == -1


# ------------------------------------------------------------------ the order of the requests (vc_create touches no device state beyond hipSetDevice)
def test_request_order_python():
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args("tiny128", num_decoder_layers=1)
    with pytest.raises(ValueError, match="w8_wide=True"):
        VoiceCraftEngine(a, {}, w8_wide=True)


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
        m = re.search(r"rows_gemm_wds_w8_k<(\d+), (\d+), (\d+)>", isa.demangle(name))
        if not m:
            continue
        seen.add(tuple(int(x) for x in m.groups()))
        assert private_segment == 0, (name, private_segment)
        assert vgpr <= 256, (name, vgpr)
        assert "v_cvt_scalef32_pk_bf16_fp8" in body, name
    assert len(seen) == 12 and {k for k, _, _ in seen} == {2, 4, 8} and {r for _, r, _ in seen} == {2, 4}, seen
