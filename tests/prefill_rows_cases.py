"""Every row of a prefill pass against the oracle: the case table of tests/test_gpu_prefill_rows.py, the recording oracle, the
row map and the checker.  No GPU in this module; tests/test_prefill_rows_cpu.py checks the table and the checker on the oracle alone.

The other parity tests read the head logits of a prompt's LAST row and of the decode steps.  Every other row of a prefill pass reaches
those only as one K/V row among hundreds in a softmax, judged on the bf16 bar - a block GEMM or attention defect that damages a few rows
passes them.  Here every row is read back: K and V of every layer from the cache (vc_debug_read "kcache<l>" / "vcache<l>"), the head
logits and per-row loss terms of every row of a teacher-forced evaluation pass (VoiceCraftEngine.forward(_per_row=True): `_logit_rows`,
`_nll_rows`), and the `emb` arena.

Row map.  The engine lays the utterances of a call back to back, each at a row that is a multiple of 16 (64 under tile_attn64_k), text
rows first, then the audio columns; padding rows carry position -1.  `layout(case)` builds that order from vc_eval_layout (evaluation
calls) or from the prompt columns the oracle exposes (TTS and editing calls) and so takes each engine row to (utterance, position), i.e.
to the oracle's K/V row and - audio rows of an evaluation call - to its logits column.

Bars (check_rows).  fp32: |d| <= 1e-3 per element where |want| < 1e3 (the bar of tests/test_gpu_scale.py) and, for logits rows, the
arg-max of every codebook.  bf16: relative L2 per row <= 2e-2 (the project's bf16 bar) over the d channels of a K or V row / the live
[K, V] logits of a logits row.  Per-row loss terms: nll = logsumexp(z) - z[target] moves by at most 2 max|dz|, so fp32 terms are held
to 2e-3 (1e-6 relative where the target is the muted terminator, |nll| ~ 1e4: an fp32 ulp there is 1e-3); in bf16 the logits row is
already judged against the oracle, and the term must equal the cross-entropy of the ENGINE'S OWN logits row and the oracle's target
within 2e-3 - which is what pins the row-to-target keying.

Census.  `expected_census(case)` restates launch_blk / launch_blk_e (vc_gemm_pf.hip) and plan_pass / make_plan (vc_engine.hip) for the
case's width, dtype and rows per pass; Case.forms is the same statement written by hand, per pass (QKV epilogue, then the form of QKV /
out-projection / FFN-up / FFN-down), and the CPU test holds the two against each other."""
from __future__ import annotations

import ctypes as C
import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from oracle.voicecraft_oracle import VoiceCraftOracle

SEED = 7
BAR_F32, BAR_BF16, BAR_NLL = 1e-3, 2e-2, 2e-3
BLK_M, BIG_M, MAX_ROWS = 128, 256, 2048          # vc_gemm_pf.hip VC_BLK_M / VC_BIG_M, vc_common.h VC_MAX_ROWS


@dataclass(frozen=True)
class Case:
    name: str
    family: str               # eval | tts | multi | edit
    preset: str               # synth preset; every model has 2 decoder layers
    dtype: str
    rows: tuple               # valid rows (text + audio positions) per utterance
    forms: tuple              # per pass: (QKV epilogue, QKV form, out-projection form, FFN-up form, FFN-down form)
    max_seqs: int = 0         # 0: the number of utterances; > 16 makes the engine pack the 16-channel QKV image (EPI_QKV16)
    max_positions: int = 512
    options: tuple = ()       # ((name, value), ...) for VoiceCraftEngine.set_option
    align: int = 16           # row alignment of an utterance in the stream (64 under tile_attn64_k)
    attn: str = "tile_attn"   # prefill attention kernel
    pins: str = ""

    @property
    def B(self):
        return len(self.rows)

    @property
    def seqs(self):
        return self.max_seqs or self.B

    @property
    def stream(self):
        return sum(-(-r // self.align) * self.align for r in self.rows)

    @property
    def pass_rows(self):
        o = dict(self.options)
        chunk = int(o.get("prefill_rows", MAX_ROWS))
        return tuple(min(chunk, self.stream - r0) for r0 in range(0, self.stream, chunk))


def _rows(tiles, slack):
    return tuple(16 * t - s for t, s in zip(tiles, slack))


def _slack(n):
    return tuple((3 + 5 * i) % 16 for i in range(n))


B64 = ("blk64",) * 4
SBS = "blk128_sbs"
BIG = "big256"
T1808, T2048, T1792 = (14, 9, 17, 12, 20, 11, 16, 14), (14, 18, 12, 20, 17, 15, 13, 19), (14, 9, 17, 12, 20, 11, 15, 14)
T2304 = (14, 18, 12, 20, 17, 15, 13, 22, 13)          # utterance 7 holds rows 1744 .. 2095: across the pass boundary at 2048 (and 1040 is inside 4)
T656, T1296 = (17, 13, 11), (14, 18, 12, 20, 17)
ODD_PRESETS = ("w768_h12", "w768_h24", "w1280_h10", "w1536_h24", "w1792_h14", "w1792_h56")
T400, T1024, T1040, T1552, T1904 = (9, 7, 9), (17, 13, 20, 14), (17, 12, 19, 14, 3), (17, 13, 20, 14, 18, 15), (14, 18, 12, 20, 17, 15, 13, 10)


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    # ---- evaluation pass: K/V of all layers, every logits row, every loss term
    small = (100, 77, 67)     # rows 0..99 | 112..188 | 192..258: an utterance boundary and padding rows inside block 0, the last block one tile of 3 rows
    for preset in ("tiny", "tiny128"):
        for dtype in ("fp32", "bf16"):
            add(f"e-small-{preset}-{dtype}", "eval", preset, dtype, small, (("QKV",) + B64,), pins="blk64, ragged last tile")
    add("e-small-tiny128-bf16-q16", "eval", "tiny128", "bf16", small, (("QKV16",) + B64,), max_seqs=17, pins="blk64 under EPI_QKV16")
    for dtype in ("fp32", "bf16"):
        f2 = SBS if dtype == "fp32" else "blk64"          # FFN-down: 4 K slices in fp32 (240 workgroups from 15 blocks), 2 in bf16
        add(f"e-sbs-512-{dtype}", "eval", "tiny128", dtype, _rows(T1808, _slack(8)), (("QKV", SBS, "blk64", SBS, f2),),
            pins="blk128_sbs at d = 512, exact mode too; last block one tile")
        add(f"e-sbs-512-full-{dtype}", "eval", "tiny128", dtype, _rows(T2048, _slack(8)), (("QKV", SBS, "blk64", SBS, f2),),
            pins="blk128_sbs at the row cap")
        add(f"e-sbs-512-edge-{dtype}", "eval", "tiny128", dtype, _rows(T1792, _slack(8)), (("QKV",) + B64,), pins="14 blocks: back on blk64")
    add("e-sbs-2048-fp32", "eval", "giga830M", "fp32", _rows(T400, _slack(3)), (("QKV", SBS, SBS, SBS, SBS),), pins="blk128_sbs in fp32 at d = 2048")
    add("e-big-1024", "eval", "giga830M", "bf16", _rows(T1024, _slack(4)), (("QKV16", SBS, SBS, SBS, SBS),), max_seqs=17,
        pins="four 256-row blocks: no big256 yet; blk128_sbs under EPI_QKV16")
    add("e-big-1040", "eval", "giga830M", "bf16", _rows(T1040, _slack(5)), (("QKV", BIG, SBS, BIG, BIG),),
        pins="big256 on QKV (12-channel image) / FFN-up / FFN-down, five blocks, the last holding 16 rows")
    add("e-big-1552", "eval", "giga830M", "bf16", _rows(T1552, _slack(6)), (("QKV16", BIG, SBS, BIG, BIG),), max_seqs=17,
        pins="seven blocks: big256 on the 16-channel QKV image")
    add("e-big-2048", "eval", "giga830M", "bf16", _rows(T2048, _slack(8)), (("QKV", BIG, SBS, BIG, BIG),), pins="eight full 256-row blocks")
    # ---- widths that are no power of two (tests/odd_width_cases.py has their decode steps): 10 .. 56 heads in the QKV epilogue's cache
    # write and in tile_attn_k's grid, K = 768 .. 1792 and 4 K in the block GEMMs; then each block form beyond blk64 at the smallest stream
    # at which the launch rules take it, at the width where that stream is cheapest
    for preset in ODD_PRESETS:
        for dtype in ("bf16", "fp32") if preset in ("w768_h12", "w1280_h10", "w1792_h56") else ("bf16",):
            add(f"e-small-{preset}-{dtype}", "eval", preset, dtype, small, (("QKV",) + B64,), pins="blk64 at an odd width, ragged last tile")
    add("e-sbs-1280-fp32", "eval", "w1280_h10", "fp32", _rows(T656, _slack(3)), (("QKV", SBS, "blk64", SBS, SBS),),
        pins="blk128_sbs at d = 1280: 40 x 6 blocks of QKV reach 240 workgroups from 641 rows on")
    add("e-big-1792", "eval", "w1792_h56", "bf16", _rows(T1296, _slack(5)), (("QKV", BIG, "blk64", BIG, BIG),),
        pins="big256 at d = 1792: 28 x 6 blocks of QKV reach 160 workgroups from 1 281 rows on; the out-projection (7 x 6) stays on blk64")
    # ---- more than one pass: rows of pass 2 attend to cache rows of pass 1; one utterance lies across the boundary
    add("e-pass-tiny128-fp32-2304", "eval", "tiny128", "fp32", _rows(T2304, _slack(9)),
        (("QKV", SBS, "blk64", SBS, SBS), ("QKV",) + B64), pins="default pass size, stream of 2 304 rows: passes of 2 048 + 256")
    add("e-pass-tiny128-fp32-1040", "eval", "tiny128", "fp32", _rows(T2304, _slack(9)), (("QKV",) + B64,) * 3,
        options=(("prefill_rows", "1040"),), pins="passes of 1 040 + 1 040 + 224 rows")
    add("e-pass-giga-bf16-1040", "eval", "giga830M", "bf16", _rows(T1552, _slack(6)), (("QKV", BIG, SBS, BIG, BIG), ("QKV", SBS, "blk64", SBS, SBS)),
        options=(("prefill_rows", "1040"),), pins="passes of 1 040 + 512 rows at giga width")
    # ---- inference calls: K/V of all layers at the prompt positions, the emb arena
    for dtype in ("fp32", "bf16"):
        add(f"p-tts-{dtype}", "tts", "tiny128", dtype, (211,), (("QKV",) + B64,), pins="tile_attn_k through the next layer's K/V rows")
    add("p-tts-bf16-attn64", "tts", "tiny128", "bf16", (211,), (("QKV",) + B64,), options=(("tile_attn", "2,128"),), align=64, attn="tile_attn64",
        pins="tile_attn64_k, ragged last 64-row block")
    add("p-multi-tiny128-fp32", "multi", "tiny128", "fp32", _rows(T1808, _slack(8)), (("QKV", SBS, "blk64", SBS, SBS),),
        options=(("shrink", "0"),), pins="the QKV epilogue's scatter to eight cache slots on blk128_sbs")
    add("p-multi-giga-bf16", "multi", "giga830M", "bf16", _rows(T1904, _slack(8)), (("QKV", BIG, SBS, BIG, BIG),),
        options=(("shrink", "0"),), pins="... on big256")
    for dtype in ("fp32", "bf16"):
        add(f"p-edit-{dtype}", "edit", "tiny128", dtype, (14 + 150 - 35 + 3 * 4 + 1 + 3 + 1,), (("QKV",) + B64,), pins="editing prompt layout: placeholders, moved pieces")
    return out


EDIT_LX, EDIT_T, EDIT_SPANS = 14, 150, ((30, 45), (90, 110))      # prompt columns: 150 - 35 kept frames, 3 pieces x K delay columns, eos, 3 placeholders, the all-empty column
CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ the engine's launch rules, restated
def _make_plan(N, Kdim, bf16, allow_split, th=16):
    """vc_engine.hip make_plan: (weight tiles, K slices)."""
    n_tiles, KT, ks = -(-N // th), Kdim // (32 if bf16 else 16), 1
    if allow_split:
        while n_tiles * ks < 512 and ks < 4 and KT // (ks * 2) >= 32 and KT % (ks * 2 * 8) == 0:
            ks *= 2
    return n_tiles, ks


def _blk_form(n_tiles, ks, rows, bf16):
    """vc_gemm_pf.hip launch_blk / launch_blk_e."""
    if bf16 and rows > 512 and n_tiles % 16 == 0 and (n_tiles // 16) * -(-rows // BIG_M) * ks >= 160:
        return BIG
    if n_tiles % 8 == 0 and (n_tiles // 8) * -(-rows // BLK_M) * ks >= 240:
        return SBS
    return "blk64"


def derived_forms(case):
    """Per pass (QKV epilogue, QKV, out-projection, FFN-up, FFN-down) from the rules above and plan_pass's choice of the QKV image."""
    d = model(case.preset)[0].d_model
    bf16 = case.dtype == "bf16"
    q12, q16 = _make_plan(3 * d, d, bf16, False, 12), _make_plan(3 * d, d, bf16, False, 16)
    po, p1, p2 = _make_plan(d, d, bf16, True), _make_plan(4 * d, d, bf16, False), _make_plan(d, 4 * d, bf16, True)
    out = []
    for rows in case.pass_rows:
        assert rows > 16, "a pass of one tile runs on the decode kernels"
        blk = -(-rows // BLK_M)
        tiles_ok = not ((q12[0] // 8) * blk >= 240 and (q16[0] // 8) * blk < 240)
        use16 = case.seqs > 16 and tiles_ok
        q = q16 if use16 else q12
        out.append(("QKV16" if use16 else "QKV", _blk_form(*q, rows, bf16), _blk_form(*po, rows, bf16), _blk_form(*p1, rows, bf16), _blk_form(*p2, rows, bf16)))
    return tuple(out)


def expected_census(case, L=2):
    """launch_counts delta of the call's PREFILL: {form: launches}.  ln_rows: two per layer and pass (+ one per 16-row head group of an
    evaluation call); the attention kernel once per layer and pass (tile_attn64_k launches count in `tile_attn` too)."""
    c = {k: 0 for k in ("blk64", SBS, BIG, "tile_attn", "tile_attn64", "ln_rows")}
    for f in case.forms:
        for form in f[1:]:
            c[form] += L
        c["tile_attn"] += L
        if case.attn == "tile_attn64":
            c["tile_attn64"] += L
        c["ln_rows"] += 2 * L
    if case.family == "eval":
        c["ln_rows"] += case.stream // 16
    return c


# ------------------------------------------------------------------------------------------------ models and inputs
@functools.lru_cache(maxsize=None)
def model(preset):
    from voicecraft_amd import synth
    a = synth.make_args(preset, num_decoder_layers=2)
    return a, synth.make_state_dict(a, seed=SEED, fast=a.d_model > 512)


def model_cfg(a, max_seqs=4, max_positions=512):
    from voicecraft_amd import _lib
    return _lib.ModelCfg(d_model=a.d_model, nhead=a.nhead, num_layers=a.num_decoder_layers, n_codebooks=a.n_codebooks,
                         audio_vocab_size=a.audio_vocab_size, n_special=int(a.n_special), text_rows=a.text_vocab_size + 1,
                         head_hidden=a.audio_vocab_size // 2, empty_token=a.empty_token, eog=a.eog, audio_pad_token=a.audio_pad_token,
                         eos=a.eos if a.eos > 0 else -1, reduced_eog=int(a.reduced_eog or 0), encodec_sr=50, max_n_spans=a.max_n_spans,
                         max_seqs=max_seqs, max_positions=max_positions)


def _n_spans(i):
    return 2 if i % 3 == 2 else 1


def _eval_extra(M, K):
    """Audio columns of a training sequence beyond its T frames: 2M + 1 pieces of K columns each, M + 1 terminators (eos > 0 with
    reduced_eog: the last kept piece and every masked piece), 2M placeholders."""
    return (2 * M + 1) * K + (M + 1) + 2 * M


@functools.lru_cache(maxsize=None)
def inputs(name):
    """eval: (xs, ys [T,K], spans per utterance); tts / multi: (xs, ys, forced [K + 1, B, K]); edit: (xs, ys, spans, forced [2 (K + 1), 1, K])."""
    c = BY_NAME[name]
    a, _ = model(c.preset)
    K = a.n_codebooks
    rs = np.random.RandomState(zlib.crc32(name.encode()))
    xs, ys, spans = [], [], []
    for i, r in enumerate(c.rows):
        if c.family == "edit":
            Lx, T = EDIT_LX, EDIT_T
        else:
            Lx = min(7 + (5 * i) % 13, r // 4)
            T = r - Lx - (_eval_extra(_n_spans(i), K) if c.family == "eval" else 1)
        assert T >= 8, (name, i, r, T)
        xs.append(torch.from_numpy(rs.randint(0, a.text_vocab_size, size=Lx).astype(np.int64)))
        ys.append(torch.from_numpy(rs.randint(0, a.audio_vocab_size, size=(T, K)).astype(np.int64)))
        spans.append([(T // 3, T // 3 + T // 4)] if _n_spans(i) == 1 else [(T // 5, T // 5 + T // 6), (T // 2, T // 2 + T // 5)])
    if c.family == "eval":
        return xs, ys, spans
    # the shortest trajectory: one plain frame, then the staggered end of the span (voicecraft.py:1057-1066), per span
    term = a.eog if c.family == "edit" else a.eos
    one = np.zeros((K + 1, c.B, K), dtype=np.int64)
    one[0] = rs.randint(0, a.audio_vocab_size, size=(c.B, K))
    for j in range(K):
        one[1 + j, :, :j] = a.empty_token
        one[1 + j, :, j] = term
    if c.family == "edit":
        return xs, ys, [list(EDIT_SPANS)], np.concatenate([one, one], axis=0)
    return xs, ys, one


def eval_batch(name):
    """The `batch` dict and mask_intervals of VoiceCraftEngine.forward / VoiceCraftOracle.forward."""
    xs, ys, spans = inputs(name)
    a, _ = model(BY_NAME[name].preset)
    B, K = len(xs), a.n_codebooks
    x_lens, y_lens = torch.tensor([len(v) for v in xs]), torch.tensor([len(v) for v in ys])
    x = torch.full((B, int(x_lens.max())), a.text_pad_token, dtype=torch.int64)
    y = torch.full((B, K, int(y_lens.max())), a.audio_pad_token, dtype=torch.int64)
    for i in range(B):
        x[i, : len(xs[i])] = xs[i]
        y[i, :, : len(ys[i])] = ys[i].t()
    return {"x": x, "x_lens": x_lens, "y": y, "y_lens": y_lens}, spans


# ------------------------------------------------------------------------------------------------ the row map
@dataclass(frozen=True)
class Layout:
    R: int                    # rows of the stream
    utt: np.ndarray           # [R] utterance of a row (= its cache slot), -1 padding
    pos: np.ndarray           # [R] position, -1 padding
    Lx: tuple                 # text rows per utterance
    row0: tuple
    tgt: np.ndarray           # eval: [R, K] target token, -1 none

    @property
    def valid(self):
        return self.pos >= 0


@functools.lru_cache(maxsize=None)
def layout(name):
    c = BY_NAME[name]
    a, sd = model(c.preset)
    K = a.n_codebooks
    inp = inputs(name)
    xs, ys = inp[0], inp[1]
    n_pos, tgts = [], []
    if c.family == "eval":
        from voicecraft_amd import _lib
        lib, cfg = _lib.load(), model_cfg(a)
        y_off = 0
        for i, sp in enumerate(inp[2]):
            Lx, T, M = len(xs[i]), len(ys[i]), len(sp)
            flat, mv = (C.c_int32 * (2 * M))(*[v for se in sp for v in se]), (C.c_int32 * M)(*range(M))
            seg, n_seg, n_cols = (C.c_int32 * (32 * 6))(), C.c_int(0), C.c_int(0)
            cap = (Lx + T + 64) * K
            tg = (C.c_int32 * cap)()
            assert lib.vc_eval_layout(C.byref(cfg), Lx, T, flat, M, mv, y_off, seg, C.byref(n_seg), C.byref(n_cols), tg, cap) == 0, (name, i)
            t = np.array(tg[: (Lx + n_cols.value) * K], dtype=np.int64).reshape(-1, K)
            flat_y = torch.cat(ys).reshape(-1).numpy()
            tok = np.where(t >= 0, flat_y[np.clip(t, 0, None)], np.where(t <= -2, -(t + 2), -1))
            n_pos.append(Lx + n_cols.value)
            tgts.append(tok)
            y_off += T
    elif c.family == "edit":
        orc = VoiceCraftOracle(a, sd)
        M = len(inp[2][0])
        _, cols, _ = orc._edit_cols(ys[0].t().unsqueeze(0), inp[2][0], list(range(a.max_n_spans))[:M] * 2)
        n_pos.append(len(xs[0]) + cols.shape[1])
    else:
        from oracle.voicecraft_oracle import prompt_columns_tts
        for x, y in zip(xs, ys):
            n_pos.append(len(x) + prompt_columns_tts(y.numpy(), a.empty_token).shape[1])
    assert tuple(n_pos) == c.rows, (name, n_pos, c.rows)
    R = c.stream
    utt, pos, tgt = np.full(R, -1), np.full(R, -1), np.full((R, K), -1, dtype=np.int64)
    row0, r = [], 0
    for i, n in enumerate(n_pos):
        row0.append(r)
        utt[r: r + n], pos[r: r + n] = i, np.arange(n)
        if tgts:
            tgt[r: r + n] = tgts[i]
        r += -(-n // c.align) * c.align
    assert r == R
    for v in (utt, pos, tgt):
        v.setflags(write=False)
    return Layout(R, utt, pos, tuple(len(x) for x in xs), tuple(row0), tgt)


# ------------------------------------------------------------------------------------------------ the recording oracle
class RowsOracle(VoiceCraftOracle):
    """VoiceCraftOracle that records, whenever a stack runs without a cache (the prefill of `inference_tts` / `inference`, the whole of
    `forward`), K and V of every layer in `self.rec[l]` ([B, H, n, hd] each) and the stack's input rows in `self.rec_in` ([B, n, d]).
    `self.defect` = (kind, layer, ...) is a defect model of tests/test_prefill_rows_cpu.py, in oracle coordinates (batch index, row):
      ("swap", l, b, r1, r2)        FFN-down of layer l leaves rows r1 and r2 exchanged
      ("copy", l, b, r, b2, r2)     ... leaves row (b2, r2) in the place of row (b, r)
      ("chunk", l, b, r, k0[, w])   ... drops the w-wide (256 unless given) K chunk at k0 from row (b, r)
      ("slot", l, b, r, b2, r2)     layer l's K/V of row (b, r) are written to slot b2 (row r2: the same position there); slot b keeps zeros"""

    def __init__(self, args, state_dict, dtype=torch.float32):
        super().__init__(args, state_dict, dtype)
        self.rec, self.rec_in, self.defect = {}, None, None

    def _attn(self, l, x, mask, past_l):
        p = f"decoder.layers.{l}.self_attn."
        B, n, d = x.shape
        H, hd = self.H, self.hd
        xt = x.transpose(1, 0)
        proj = F.linear(xt, self.sd[p + "in_proj_weight"], self.sd[p + "in_proj_bias"])
        proj = proj.unflatten(-1, (3, d)).unsqueeze(0).transpose(0, -2).squeeze(-2).contiguous()
        q, k, v = (t.view(n, B * H, hd).transpose(0, 1).view(B, H, n, hd) for t in (proj[0], proj[1], proj[2]))
        present = torch.stack([k, v], dim=0)
        if past_l is not None:
            k = torch.cat([past_l[0], k], dim=-2)
            v = torch.cat([past_l[1], v], dim=-2)
        else:
            if self.defect and self.defect[0] == "slot" and self.defect[1] == l:
                _, _, b, r, b2, r2 = self.defect
                k, v = k.clone(), v.clone()
                for t in (k, v):
                    t[b2, :, r2] = t[b, :, r]
                    t[b, :, r] = 0
            self.rec[l] = (k.clone(), v.clone())
        o = F.scaled_dot_product_attention(q, k, v, mask, 0.0, is_causal=False)
        o = o.permute(2, 0, 1, 3).contiguous().view(B * n, d)
        o = F.linear(o, self.sd[p + "out_proj.weight"], self.sd[p + "out_proj.bias"]).view(n, B, d)
        return o.transpose(1, 0), present

    def _stack(self, x, mask, past):
        if past is None:
            self.rec_in = x.clone()
        pres = []
        for l in range(self.L):
            p = f"decoder.layers.{l}."
            a, pr = self._attn(l, F.layer_norm(x, (self.d,), self.sd[p + "norm1.weight"], self.sd[p + "norm1.bias"], 1e-5),
                               mask, None if past is None else past[l])
            x = x + a
            h = F.layer_norm(x, (self.d,), self.sd[p + "norm2.weight"], self.sd[p + "norm2.bias"], 1e-5)
            act = F.relu(F.linear(h, self.sd[p + "linear1.weight"], self.sd[p + "linear1.bias"]))
            h = F.linear(act, self.sd[p + "linear2.weight"], self.sd[p + "linear2.bias"])
            if past is None and self.defect and self.defect[1] == l and self.defect[0] != "slot":
                h = h.clone()
                if self.defect[0] == "swap":
                    _, _, b, r1, r2 = self.defect
                    h[b, [r1, r2]] = h[b, [r2, r1]]
                elif self.defect[0] == "copy":
                    _, _, b, r, b2, r2 = self.defect
                    h[b, r] = h[b2, r2]
                else:
                    _, _, b, r, k0 = self.defect[:5]
                    k1 = k0 + (self.defect[5] if len(self.defect) > 5 else 256)
                    h[b, r] = h[b, r] - self.sd[p + "linear2.weight"][:, k0: k1] @ act[b, r, k0: k1]
            x = x + h
            pres.append(pr)
        x = F.layer_norm(x, (self.d,), self.sd["decoder.norm.weight"], self.sd["decoder.norm.bias"], 1e-5)
        return x, torch.stack(pres, dim=0)


def oracle_rows(name, dtype=torch.float32, defect=None):
    """One oracle run of the case, re-ordered into the engine's rows: {"k" / "v": [L][R, d], "emb": [R, d], and for evaluation calls
    "logits": [R, K, V] (zero rows where the oracle has none: text and padding rows), "has_logits": [R], "nll": [R, K]}; float64
    numpy arrays when dtype is float64, else float32.  `defect`: a RowsOracle defect in ENGINE coordinates - utterance numbers and
    positions - translated here."""
    c = BY_NAME[name]
    a, sd = model(c.preset)
    lay = layout(name)
    orc = RowsOracle(a, sd, dtype)
    K, d, L = a.n_codebooks, a.d_model, a.num_decoder_layers
    inp = inputs(name)
    xs, ys = inp[0], inp[1]
    recs, ins, logit_cols, off = [], [], None, None
    if c.family == "eval":
        batch, spans = eval_batch(name)
        Lmax = int(batch["x_lens"].max())
        o_row = lambda u, p: p if p < lay.Lx[u] else Lmax + p - lay.Lx[u]          # the oracle pads the texts to the longest
        if defect:
            kind, l, u, p = defect[:4]
            orc.defect = {"swap": lambda: (kind, l, u, o_row(u, p), o_row(u, defect[4])),
                          "copy": lambda: (kind, l, u, o_row(u, p), defect[4], o_row(defect[4], defect[5])),
                          "chunk": lambda: (kind, l, u, o_row(u, p), defect[4]),
                          "slot": lambda: (kind, l, u, o_row(u, p), defect[4], o_row(defect[4], p))}[kind]()
        ref = orc.forward(batch, spans)
        logit_cols = ref["_logits_cols"]
        recs, ins = [orc.rec] * c.B, [orc.rec_in] * c.B
        off = [(u, Lmax) for u in range(c.B)]
    else:
        assert defect is None
        for u in range(c.B):
            x, y = xs[u].unsqueeze(0), ys[u].unsqueeze(0)
            if c.family == "edit":
                mi = torch.tensor([inp[2][0]], dtype=torch.int64)
                orc.inference(x, torch.tensor([x.shape[1]]), y, mi, top_k=1, forced=inp[3][:, 0])      # runs to its end: the trajectory is one the call accepts
            else:
                orc.inference_tts(x, torch.tensor([x.shape[1]]), y, top_k=1, forced=inp[2][:, u], max_steps=1)
            recs.append(orc.rec)
            ins.append(orc.rec_in)
            orc.rec = {}
        off = [(0, lay.Lx[u]) for u in range(c.B)]
    npdt = np.float64 if dtype == torch.float64 else np.float32
    out = {"k": [np.zeros((lay.R, d), npdt) for _ in range(L)], "v": [np.zeros((lay.R, d), npdt) for _ in range(L)], "emb": np.zeros((lay.R, d), npdt)}
    for u in range(c.B):
        n, r0, Lx = c.rows[u], lay.row0[u], lay.Lx[u]
        b, Lpad = off[u]
        idx = np.concatenate([np.arange(Lx), Lpad + np.arange(n - Lx)])
        for l in range(L):
            for key, t in zip(("k", "v"), recs[u][l]):
                out[key][l][r0: r0 + n] = t[b][:, idx].permute(1, 0, 2).reshape(n, d).numpy()          # [H, n, hd] -> head-major rows
        out["emb"][r0: r0 + n] = ins[u][b, idx].numpy()
    if logit_cols is not None:
        V = logit_cols.shape[-1]
        lg, has, nll = np.zeros((lay.R, K, V), npdt), np.zeros(lay.R, bool), np.zeros((lay.R, K), npdt)
        for u in range(c.B):
            n, r0, Lx = c.rows[u], lay.row0[u], lay.Lx[u]
            cols = logit_cols[u, :, : n - Lx]                                   # [K, n - Lx, V]
            lg[r0 + Lx: r0 + n] = cols.permute(1, 0, 2).numpy()
            has[r0 + Lx: r0 + n] = True
            tg = torch.from_numpy(lay.tgt[r0 + Lx: r0 + n].T.copy())             # [K, n - Lx]
            for k in range(K):
                m = tg[k] >= 0
                if m.any():
                    nll[r0 + Lx: r0 + n, k][m.numpy()] = F.cross_entropy(cols[k][m], tg[k][m], reduction="none").numpy()
        out.update(logits=lg, has_logits=has, nll=nll)
    return out


@functools.lru_cache(maxsize=3)
def reference(name):
    """The clean fp32 oracle rows of a case, shared by the tests of a process: read-only."""
    ref = oracle_rows(name)
    for v in ref.values():
        for t in (v if isinstance(v, list) else [v]):
            t.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------------ the checker
def row_error(got, want, dtype):
    """Per row: fp32 the largest |d| over the live entries (|want| < 1e3), bf16 the relative L2 over them."""
    n = len(want)
    got, want = np.asarray(got, dtype=np.float64).reshape(n, -1), np.asarray(want, dtype=np.float64).reshape(n, -1)
    live = np.abs(want) < 1e3
    diff = np.where(live, got - want, 0.0)
    diff = np.where(np.isfinite(diff), diff, np.inf)
    if dtype == "fp32":
        return np.abs(diff).max(axis=1)
    den = np.sqrt((np.where(live, want, 0.0) ** 2).sum(axis=1))
    return np.sqrt((diff ** 2).sum(axis=1)) / np.where(den > 0, den, 1.0)


def check_rows(got, want, dtype, valid, logits=False):
    """Compares EVERY row of `valid` (bool [R]; no valid row is left out).  Returns (rows over the bar, worst row, its figure).
    logits: the rows are [K, V] head logits - in fp32 the arg-max of every codebook must match as well."""
    valid = np.asarray(valid, bool)
    assert len(got) == len(want) == len(valid), (len(got), len(want), len(valid))
    err = np.where(valid, row_error(got, want, dtype), 0.0)
    bad = err > (BAR_F32 if dtype == "fp32" else BAR_BF16)
    if logits and dtype == "fp32":
        bad |= valid & (np.asarray(got).argmax(axis=-1) != np.asarray(want).argmax(axis=-1)).any(axis=-1)
    worst = int(err.argmax())
    return np.flatnonzero(bad), worst, float(err[worst])


def nll_error(got, want):
    """|d| of per-row loss terms, scaled so that the bar is BAR_NLL everywhere: plain below |want| = 1e3, 1e-6 relative above (muted targets)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.where(np.abs(want) < 1e3, 1.0, np.abs(want) * 1e-6 / BAR_NLL)


def own_nll(logit_rows, tgt):
    """Cross-entropy of logits rows [R, K, V] at the targets [R, K] (-1: none -> 0), in float64."""
    z = torch.from_numpy(np.asarray(logit_rows, np.float64))
    t = torch.from_numpy(np.array(tgt))
    out = torch.zeros(t.shape, dtype=torch.float64)
    m = t >= 0
    out[m] = F.cross_entropy(z[m], t[m], reduction="none")
    return out.numpy()
