"""Option `w8q` without a GPU: the "w8q" pairs of the 12-channel QKV image (csrc/vc_w8.h) through the host packer against
quant.w8q_decode and a numpy restatement of pack_k's th = 12 layout, the plan (vc_debug_w8q_plan: plan_pass itself with Wqkv taken as
packed) for EVERY model width the engine accepts, rows 1..64 and masks 0 / 4 / 12 against vc_debug_plan and vc_debug_w8r_plan, the new
symbols, the order of the requests, the compiled kernels (nine rows_gemm_qkvq_w8_k instantiations, no scratch, the E4M3 conversion in
each), the neighbouring plans, which must report what they reported, and the format's host round trip under a sanitizer
(tools/w8_qkv_check.cpp, a stand-alone program)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from voicecraft_amd import _lib, quant, synth
from test_w8_mid_cpu import w8m_plan
from test_w8_rows_cpu import w8r_plan
from test_w8_up_cpu import w8u_plan
from test_w8_up_rows_cpu import w8ur_plan
from test_w8_wide_cpu import OFF_GRID, ROOT, WIDTHS, cfg, image_plan, isa, w8w_plan      # (isa: tools/isa_store_scan.py)

MASKS = (0, 4, 12)
# the row counts at which the form is taken without bit 8 where it exists (csrc/vc_engine_host.h W8_FORMS, row `w8q`, from profiles/w8_qkv_rows_ab.log)
ROWS_WIN = range(5, 17)       # 5..8: measured at 7 and 8 (two tiles per workgroup); 9..16: at 9, 12, 16; 2..4 (one tile) were not measured
KTW = {512: 4, 1024: 8, 2048: 16}                 # K = d over the four waves of a tile, in k-tiles of 32 inputs, one chunk


def w8q_plan(d, h, mask, rows):
    c = cfg(d, h)
    out = (C.c_int32 * 2)()
    assert _lib.load().vc_debug_w8q_plan(C.byref(c), mask, rows, out) == 0
    return list(out)


def test_abi_new_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vc_engine.h")).read()
    for name in ("vc_request_w8_qkv_rows", "vc_debug_w8q_plan", "vc_w8q_pack_host"):
        fn = getattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert fn.restype is res and list(fn.argtypes) == args
        assert f"int {name}(" in header


# ------------------------------------------------------------------ the packer
def image12(w):
    """pack_k's th = 12 layout of a bf16-valued fp32 matrix [N, K]: [tile, k-tile, slot, value], slot s = kg * 12 + m = channel
    12 nt + m, inputs 32 kt + 8 kg .. + 7; as pairs [n_pairs, 2, 48, 8] (k-tiles 2j, 2j + 1 of one tile, tile major)."""
    n, k = w.shape
    assert n % 12 == 0 and k % 64 == 0
    slot = np.arange(48)
    img = np.empty((n // 12, k // 32, 48, 8), np.float32)
    for nt in range(n // 12):
        for kt in range(k // 32):
            rows = 12 * nt + slot % 12
            cols = 32 * kt + 8 * (slot // 12)
            img[nt, kt] = w[rows[:, None], cols[:, None] + np.arange(8)[None, :]]
    return img.reshape(-1, 2, 48, 8)


def pack_host(pairs, kt):
    """float32 pairs [n, 2, 48, 8] of bf16 values of an image of kt k-tiles per tile -> (planes uint8 [n, 768], side uint8 [n, 2], refused pairs)"""
    bits = torch.from_numpy(np.ascontiguousarray(pairs)).bfloat16().view(torch.int16).contiguous()
    assert bool((bits.view(torch.bfloat16).float() == torch.from_numpy(np.ascontiguousarray(pairs))).all())
    n = pairs.shape[0]
    planes = torch.full((n, 768), 0xAA, dtype=torch.uint8)
    side = torch.full((n, 2), 0xAA, dtype=torch.uint8)
    refused = C.c_int32(-1)
    rc = _lib.load().vc_w8q_pack_host(C.c_void_p(bits.data_ptr()), n, C.c_void_p(planes.data_ptr()), C.c_void_p(side.data_ptr()), kt,
                                      C.byref(refused))
    assert rc == 0
    return planes, side, refused.value


def part_amax(pairs, kt):
    """[pair, part]: the largest magnitude of each part, from the definition: an even tile's part 1 is m >= 8, an odd tile's m >= 4."""
    m = np.arange(48) % 12
    out = np.zeros((pairs.shape[0], 2))
    for p in range(pairs.shape[0]):
        odd = (p // (kt // 2)) & 1
        in1 = m >= (4 if odd else 8)
        out[p, 0] = np.abs(pairs[p][:, ~in1]).max()
        out[p, 1] = np.abs(pairs[p][:, in1]).max()
    return out


def check_round_trip(q):
    kt = q.shape[1] // 32
    pairs = image12(q)
    assert pairs.shape[0] == q.shape[0] // 12 * (q.shape[1] // 64)
    planes, side, refused = pack_host(pairs, kt)
    assert refused == 0
    back = quant.w8q_decode(planes, side, kt).numpy()
    assert back.shape == pairs.shape and np.array_equal(back.view(np.uint32), pairs.view(np.uint32))
    # the side bytes are the smallest shifts that hold the parts: a part's maximum in E4M3's top binade (256 .. 448), or 240 where 480
    # would be the NaN code - on both tile parities
    amax = part_amax(pairs, kt)
    parities = set()
    for p in range(pairs.shape[0]):
        parities.add((p // (kt // 2)) & 1)
        for h in range(2):
            s = int(side[p, h]) - 127
            assert amax[p, h] == 0 or 240.0 * 2.0 ** s <= amax[p, h] <= 448.0 * 2.0 ** s, (p, h, s, amax[p, h])
    assert parities == {0, 1}
    return side


@pytest.mark.parametrize("shape", [(48, 128), (72, 256)])
def test_packer_round_trip_on_quantised_matrices(shape):
    g = torch.Generator().manual_seed(5 + shape[0])
    # rows of very different magnitude, so that the blocks' shifts differ
    w = (torch.randn(shape, generator=g) * torch.logspace(-3, 1, shape[0])[:, None]).bfloat16().float()
    side = check_round_trip(quant.quantize_image(w).numpy())
    assert (side[:, 0] != side[:, 1]).any()          # the parts of a pair carry their own shifts


def test_packer_round_trip_on_a_quantised_checkpoint():
    """The (1536, 512) QKV matrix of tiny128 out of quantize_state_dict_w8: its folded image packs whole."""
    a = synth.make_args("tiny128", num_decoder_layers=2)
    sdq = quant.quantize_state_dict_w8(a, synth.make_state_dict(a, seed=0, fast=True))
    img = quant.fold(sdq["decoder.layers.1.self_attn.in_proj_weight"], sdq["decoder.layers.1.norm1.weight"])
    assert tuple(img.shape) == (1536, 512)
    check_round_trip(img.numpy())


def test_packer_parts_two_to_the_six_apart():
    m = np.arange(48) % 12
    for odd in (0, 1):
        pairs = np.zeros((2, 2, 48, 8), np.float32)      # kt = 2: pair 0 is tile 0 (even), pair 1 is tile 1 (odd)
        in1 = m >= (4 if odd else 8)
        pairs[odd][:, ~in1] = 1.5
        pairs[odd][:, in1] = 1.5 * 64.0
        planes, side, refused = pack_host(pairs, 2)
        assert refused == 0
        assert int(side[odd, 1]) - int(side[odd, 0]) == 6
        assert int(side[odd, 0]) - 127 == 0 - 8          # 1.5 = 384 . 2^-8: the top binade
        assert np.array_equal(quant.w8q_decode(planes, side, 2).numpy(), pairs)
        assert len(set(planes[odd].tolist())) == 1       # the same code everywhere: the magnitudes live in the side bytes


@pytest.mark.parametrize("tile,channel", [(0, 3), (0, 10), (1, 2), (1, 7)])
def test_packer_refuses_exactly_the_pair_with_an_off_grid_value(tile, channel):
    """OFF_GRID once in a whole-block part and once in a four-channel part, for an even and an odd tile."""
    w = quant.quantize_image(torch.randn(24, 256, generator=torch.Generator().manual_seed(3)).bfloat16().float())
    w[12 * tile + channel, 70] = OFF_GRID            # inputs 64..127: pair tile * 4 + 1
    assert float(torch.tensor(OFF_GRID).bfloat16()) == OFF_GRID
    pairs = image12(w.numpy())
    planes, side, refused = pack_host(pairs, 8)
    assert refused == 1
    back = quant.w8q_decode(planes, side, 8).numpy()
    hit = tile * 4 + 1
    wrong = [p for p in range(pairs.shape[0]) if not np.array_equal(back[p].view(np.uint32), pairs[p].view(np.uint32))]
    assert wrong == [hit], wrong
    # ... and tile by tile (a pair's parity comes with its tile): only that pair is refused
    for t in range(2):
        _, _, r = pack_host(np.concatenate([np.zeros((4 * t, 2, 48, 8), np.float32), pairs[4 * t:4 * t + 4]]), 8)
        assert r == (1 if t == tile else 0), t


def test_packer_pair_of_zeros_takes_shift_zero():
    planes, side, refused = pack_host(np.zeros((2, 2, 48, 8), np.float32), 2)
    assert refused == 0 and side.tolist() == [[127, 127], [127, 127]] and int(planes.max()) == 0
    neg = np.zeros((2, 2, 48, 8), np.float32)
    neg[1, 1, 9, 3] = -0.0
    planes, side, refused = pack_host(neg, 2)
    assert refused == 0 and side.tolist() == [[127, 127], [127, 127]]
    assert np.array_equal(quant.w8q_decode(planes, side, 2).numpy().view(np.uint32), neg.view(np.uint32))


def test_packer_bad_arguments():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    r = C.c_int32(0)
    assert lib.vc_w8q_pack_host(None, 1, buf, buf, 2, C.byref(r)) == -1
    assert lib.vc_w8q_pack_host(buf, 1, None, buf, 2, C.byref(r)) == -1
    assert lib.vc_w8q_pack_host(buf, 1, buf, None, 2, C.byref(r)) == -1
    assert lib.vc_w8q_pack_host(buf, 1, buf, buf, 2, None) == -1
    assert lib.vc_w8q_pack_host(buf, -1, buf, buf, 2, C.byref(r)) == -1
    for kt in (0, 1, 3, -2):
        assert lib.vc_w8q_pack_host(buf, 1, buf, buf, kt, C.byref(r)) == -1
    assert lib.vc_w8q_pack_host(buf, 1, buf, buf, 4, C.byref(r)) == -1          # no whole tile: two pairs per tile at KT = 4
    assert lib.vc_w8q_pack_host(buf, 2, buf, buf, 4, C.byref(r)) == 0


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("d,h", WIDTHS)
def test_w8q_plan_every_width(d, h):
    for rows in range(1, 65):
        img = image_plan(d, h, rows)
        # include/vc_engine.h vc_debug_plan: [1] form (1 = finished rows), [9] = 2 where the paired consumer (rows_gemm_qp_k) takes the
        # QKV projection of these rows.  The consumers read the centred copy (option hq, the default) where a bf16 row is whole 1 KB
        # requests of a wave: d a multiple of 512
        hq = d % 512 == 0 and 2 * d <= 8192
        paired = img[9] == 2
        may = img[1] == 1 and hq and d in KTW and not paired
        if d in KTW and 2 <= rows <= 16:
            assert paired == (rows <= (6 if d == 2048 else 8)), (d, rows, img)
            assert bool(w8r_plan(d, h, 4, rows)[1]) <= paired      # `w8r` streams the QKV bytes only where the paired consumer runs
        for mask in MASKS:
            took, k = w8q_plan(d, h, mask, rows)
            want = bool(may and (mask & 4) and ((mask & 8) or rows in ROWS_WIN))
            assert took == int(want) and k == (KTW[d] if want else 0), (d, rows, mask, took, k)
            if rows == 1 or rows >= 17 or mask == 0 or paired:
                assert [took, k] == [0, 0]


def test_w8q_plan_widths_with_a_form():
    """Bit 8 takes the form at 9..16 rows at the three widths, and at 7 and 8 rows at d = 2048 alone."""
    for rows in range(2, 17):
        by_d = {d: w8q_plan(d, h, 12, rows) for d, h in WIDTHS}
        took = {d: v[1] for d, v in by_d.items() if v[0]}
        assert took == (KTW if rows >= 9 else {2048: 16} if rows >= 7 else {}), (rows, by_d)
    # without bit 8: exactly the rows of the committed table (where the paired consumer does not take them)
    for d, h in WIDTHS:
        if d in KTW:
            lo = 7 if d == 2048 else 9
            assert [r for r in range(1, 65) if w8q_plan(d, h, 4, r)[0]] == [r for r in ROWS_WIN if lo <= r <= 16], d


def test_w8q_plan_bad_arguments():
    lib = _lib.load()
    c = cfg(2048, 16)
    out = (C.c_int32 * 2)()
    for rows in (0, -3, 65):
        assert lib.vc_debug_w8q_plan(C.byref(c), 4, rows, out) == -1
    for mask in (1, 2, 3, 5, 8, 10, 13, 16, 20, -1):
        assert lib.vc_debug_w8q_plan(C.byref(c), mask, 12, out) == -1
    assert lib.vc_debug_w8q_plan(None, 4, 12, out) == -1
    assert lib.vc_debug_w8q_plan(C.byref(c), 4, 12, None) == -1


def test_neighbouring_plans_report_what_they_reported():
    """`w8r` keeps the paired consumer's row counts, `w8m` covers 9..16 with the FFN down-projection, `w8ur` 2..16 with FFN-up, `w8w`
    and `w8u` start at 17 rows: none of them moved."""
    # (the values tests/test_w8_mid_cpu.py pins)
    assert w8r_plan(2048, 16, 5, 6) == [1, 1, 4, 1] and w8r_plan(2048, 16, 5, 8) == [1, 0, 4, 0] and w8r_plan(2048, 16, 5, 9) == [0, 0, 0, 0]
    assert w8u_plan(2048, 16, 10, 16) == [0, 0] and w8u_plan(2048, 16, 2, 17) == [1, 8] and w8u_plan(512, 8, 10, 64) == [1, 2]
    assert w8w_plan(2048, 16, 5, 16) == [0, 0, 0, 0] and w8w_plan(2048, 16, 5, 17) == [1, 1, 8, 8]
    assert w8w_plan(1024, 16, 13, 17) == [1, 1, 4, 4]
    assert w8m_plan(2048, 16, 1, 8) == [0, 0, 0, 0] and w8m_plan(2048, 16, 1, 9) == [1, 2, 2, 0] and w8m_plan(2048, 16, 1, 17) == [0, 0, 0, 0]
    assert w8m_plan(512, 8, 9, 16) == [1, 1, 1, 0] and w8m_plan(1024, 16, 1, 12) == [1, 1, 2, 0]
    assert w8ur_plan(2048, 16, 2, 12) == [1, 16] and w8ur_plan(1024, 16, 2, 2) == [1, 8] and w8ur_plan(512, 8, 2, 17) == [0, 0]


# ------------------------------------------------------------------ the order of the requests
def test_request_order():
    """ValueError without `w8=`; the C request on a null handle; and on a bare handle where vc_create gives one (it selects a device and
    touches nothing else, so it needs one: tests/test_gpu_w8_qkv_rows.py repeats the walk where a GPU is certain)."""
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args("tiny128", num_decoder_layers=1)
    with pytest.raises(ValueError, match="w8_qkv_rows=True"):
        VoiceCraftEngine(a, {}, w8_qkv_rows=True)
    assert VoiceCraftEngine.W8_QKV_ROWS_MASK == 4 and VoiceCraftEngine.LAUNCH_FORMS[-1] == "w8_up"
    assert VoiceCraftEngine.LAUNCH_FORMS_MORE == ("w8_up_rows",) and VoiceCraftEngine.LAUNCH_FORMS_MORE2 == ("w8_qkv_rows",)
    lib = _lib.load()
    assert lib.vc_request_w8_qkv_rows(None, 4) == -1
    h = C.c_void_p()
    c_ = cfg(a.d_model, a.nhead)
    if lib.vc_create(C.byref(c_), 0, C.byref(h)) == 0:
        try:
            assert lib.vc_request_w8_qkv_rows(h, 4) == -2           # VC_ESTATE: after vc_request_w8 only
            assert lib.vc_request_w8(h, 5) == 0
            for bad in (0, 1, 2, 5, 8, 12, -1):
                assert lib.vc_request_w8_qkv_rows(h, bad) == -1     # VC_EINVAL
            assert lib.vc_request_w8_mid(h, 4) == -1                # bit 4 stays no bit of `w8m`
            assert lib.vc_request_w8_qkv_rows(h, 4) == 0
            assert lib.vc_request_w8_up_rows(h, 2) == 0             # the requests do not exclude each other
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
        m = re.search(r"rows_gemm_qkvq_w8_k<(\d+), (\d+), (true|false)>", isa.demangle(name))
        if not m:
            continue
        seen.add((int(m.group(1)), int(m.group(2)), m.group(3) == "true"))
        assert private_segment == 0, (name, private_segment)
        assert vgpr <= 256, (name, vgpr)
        assert "v_cvt_scalef32_pk_bf16_fp8" in body, name
    assert seen == {(k, n, r2) for k in (4, 8, 16) for n, r2 in ((1, False), (2, False), (2, True))}, seen


# ------------------------------------------------------------------ the format's host text under a sanitizer
def test_host_round_trip_under_a_sanitizer(tmp_path):
    """tools/w8_qkv_check.cpp: a stand-alone program (its own main) on csrc/vc_w8.h's plain C++, built with the host compiler and
    -fsanitize=address,undefined: random on-grid and off-grid pairs of both tile parities."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "w8_qkv_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "w8_qkv_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and re.fullmatch(r"ok \d+ \d+\n", r.stdout), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    n, refused = map(int, r.stdout.split()[1:])
    assert n > 4000 and 0 < refused < n
