"""Shared text prefix (vc_tts_multi shared_text_prefix): the case table of tests/test_gpu_shared_prefix.py and, from the
oracle alone, how far the MILDEST fault of the redirect would move each case's logits.  No GPU in this module.

Every sequence of a sentence-chained call reads cache positions < P from sequence 0's cache.  A case is one call: B texts that share
their first P phonemes and differ from index P on, sentences of different lengths (so the row tiles of sequences u > 0 start at
different offsets), one audio prompt of T frames, N samples per text, teacher-forced on random tokens.  Each case also has a STALE
call of the same shapes on entirely different text and another audio prompt: run first, without sharing, it leaves every slot's own
cache holding another call's K/V below P - without it a boundary that is one too low reads correct or zero rows and cannot be seen.

Defect models (PrefixOracle): the oracle with K/V rows substituted whenever they are READ, in the prefill and in every cached step,
  M1  position P   from sequence 0's run          - the boundary one too high            (sequences of texts u > 0)
  M2  position P-1 from the stale call's run      - the boundary one too low             (every slot but 0)
  M3  position P   from the stale call's run      - best-of-N: the sibling copy starts one row late   (samples j > 0)
defect_floor(case) is the smallest relative L2 distance between any model's head logits and the clean oracle's over every slot and
compared step: what the mildest modelled fault does.  The synthetic checkpoints attend almost uniformly, so one wrong row out of S
moves the logits by roughly 1 / S: the floor falls with the context, which every case therefore keeps at or below about 150."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from oracle.voicecraft_oracle import VoiceCraftOracle

FLOOR_MIN = 2e-3          # every case's floor must reach this (tests/test_shared_prefix_cpu.py)
KW = {"fp32": 16, "bf16": 32}          # keys per key tile of tile_attn_k
SEED = 5                  # synth.make_state_dict seed of every case
FORM_FR, FORM_WIDE = 1, 2          # vc_debug_plan out[1]


def rel_l2(got, want):
    """test_gpu_model.rel_l2: per-step relative L2 of the head logits without the muted terminator column."""
    live = np.abs(want) < 1e3
    num = np.sqrt((((got - want) * live) ** 2).reshape(len(want), -1).sum(1))
    den = np.sqrt(((want * live) ** 2).reshape(len(want), -1).sum(1))
    return num / den


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    preset: str
    dtype: str
    P: int                    # shared text prefix
    lens: tuple               # sentence length per text: text u has P + lens[u] phonemes
    T: int = 8                # frames of the audio prompt
    N: int = 1                # samples per text (best-of-N): slot u * N + j
    options: tuple = ()       # ((name, value), ...) for VoiceCraftEngine.set_option
    census: tuple = ()        # ((launch_counts slot, True: must be launched / False: must not), ...) around the call with reuse
    steps: int = 6            # compared decode steps (step 0 carries the whole prefill)
    ends: tuple = ()          # per slot: the step whose forced token is the terminator (default: `steps`, i.e. after the compared ones)
    plan: tuple = ()          # (rows, form, attention splits) the engine must plan for the decode steps (vc_debug_plan), if the case is about them

    @property
    def B(self):
        return len(self.lens)

    @property
    def slots(self):
        return self.B * self.N

    @property
    def context(self):
        """Longest cached context a compared step reads."""
        return self.P + max(self.lens) + self.T + 1 + self.steps - 1

    def end(self, s):
        return self.ends[s] if self.ends else self.steps

    def n_steps(self, s, K):
        """Compared steps of slot s: up to the last step of its staggered end."""
        return min(self.steps, self.end(s) + K)


# ------------------------------------------------------------------------------------------------ the table
# Prefill, tile_attn_k.  Key tile b = P // KW holds the boundary (none when KW divides P: then tile b - 1 comes WHOLE from sequence 0's
# cache - the fast-path branch no test ran before).  The first row tile of a sequence u > 0 covers positions P .. P + 15 at most, so
# with P % KW + 15 < KW - 1 (bf16 33 / 65; fp32 with a sentence of <= 6 phonemes, whose only tile has < 16 rows) the causal mask cuts
# the boundary tile too; a sentence of >= 8 phonemes has a second row tile, which sees the boundary in a FULL key tile; and tile b
# belongs to wave b % 4 and is that wave's last one (contexts < 5 KW): a wave other than wave 0 for every P >= KW.
_LENS = ((7, 3, 12), (4, 14, 5), (11, 2, 9))          # (text 0, a short one, a long one) in three arrangements


def _prefill_cases():
    out = []
    for dtype, presets, ps in (("fp32", ("tiny", "tiny128"), (15, 16, 17, 32, 33)), ("fp32", ("tiny128",), (63, 64, 65)),
                               ("bf16", ("tiny128", "tiny_h16", "tiny"), (31, 32, 33, 64, 65))):
        for ip, preset in enumerate(presets):
            for i, P in enumerate(ps):
                out.append(Case(f"pf-{preset}-{dtype}-P{P}", "prefill", preset, dtype, P, _LENS[(i + ip) % 3],
                                census=(("tile_attn", True), ("tile_attn64", False))))
    # tile_attn64_k: 64-row blocks; every prompt has >= 64 rows after the skip (text 1: exactly 64, text 2: 67 - a ragged last block).
    # 64 rows behind a prefix of 65 are a context of ~130, where the floor is at its limit: the sentences are as short as they go and
    # only the prefill step and one decode step are compared.
    for P in (31, 33, 63, 64, 65):
        out.append(Case(f"pf64-tiny128-bf16-P{P}", "prefill64", "tiny128", "bf16", P, (2, 1, 4), T=62, options=(("tile_attn", "2,64"),),
                        census=(("tile_attn64", True),), steps=2))
    # passes of 64 rows: text 0 takes 80 / 112 rows (padded), so its prefix is prefilled in pass 0 and the other texts' rows in later ones
    out.append(Case("pfpass-tiny128-fp32-P33", "multipass", "tiny128", "fp32", 33, (7, 4, 10), T=24, options=(("prefill_rows", "64"),),
                    census=(("tile_attn", True), ("tile_attn64", False))))
    out.append(Case("pfpass-tiny128-bf16-P65", "multipass", "tiny128", "bf16", 65, (7, 4, 10), T=24, options=(("prefill_rows", "64"),),
                    census=(("tile_attn", True), ("tile_attn64", False))))
    return out


def _rows_lens(rows):
    return tuple(3 + (5 * u) % 11 for u in range(rows))


def _decode_cases():
    """rows_attn_k, general form (share != 0).  Rows of a step = sequences of the call: 2 / 3 / 8 rows run 8 / 4 / 2 attention splits
    (bf16: partials in bf16, option att_p16, or in fp32), 10 rows the unsplit finished-row form, 20 rows the wide form."""
    out = []
    splits = {2: 8, 3: 4, 8: 2, 10: 1, 20: 1}
    for rows in (2, 3, 8, 10, 20):
        plan = (rows, FORM_WIDE if rows > 16 else FORM_FR, splits[rows])
        census = (("rows_attn", True), ("wd", rows > 16))
        for dtype in ("bf16", "fp32"):
            for preset, P in (("tiny128", 33), ("tiny_h16", 65)) if dtype == "bf16" else (("tiny128", 65), ("tiny_h16", 33)):
                out.append(Case(f"dec{rows}-{preset}-{dtype}-P{P}", "decode", preset, dtype, P, _rows_lens(rows), census=census, plan=plan))
                if dtype == "bf16" and rows <= 3:
                    out.append(Case(f"dec{rows}-{preset}-bf16-P{98 - P}-p32", "decode", preset, "bf16", 98 - P, _rows_lens(rows),
                                    options=(("att_p16", "0"),), census=census, plan=plan))
    for dtype, P in (("bf16", 65), ("fp32", 33)):
        out.append(Case(f"dec3-tiny-{dtype}-P{P}", "decode", "tiny", dtype, P, _rows_lens(3), census=(("rows_attn", True), ("wd", False)),
                        plan=(3, FORM_FR, 4)))
    # the refill loop: unsplit, so a row's chunk is its whole context > 4 * 8 * PPW positions (128 at head_dim 128 in bf16, 64 in fp32):
    # the boundary lies in a refilled batch.  At 131 the context is ~140 and the floor is at its limit: the audio prompt and the
    # sentences are as short as they go, and fewer steps are compared.
    refill = (("rows_attn", True), ("wd", False))
    out.append(Case("refill10-tiny128-bf16-P131", "refill", "tiny128", "bf16", 131, tuple(1 + u % 3 for u in range(10)), T=2, steps=4,
                    census=refill, plan=(10, FORM_FR, 1)))
    out.append(Case("refill10-tiny128-fp32-P131", "refill", "tiny128", "fp32", 131, tuple(1 + u % 2 for u in range(10)), T=1, steps=3,
                    census=refill, plan=(10, FORM_FR, 1)))
    out.append(Case("refill10-tiny128-fp32-P67", "refill", "tiny128", "fp32", 67, _rows_lens(10), census=refill, plan=(10, FORM_FR, 1)))
    # retirement: text 0 ends at step 4 and leaves the batch (re-packed with option shrink) while the others still read its prefix
    for preset, dtype in (("tiny128", "bf16"), ("tiny_h16", "fp32")):
        for shrink in ("1", "0"):
            out.append(Case(f"retire-{preset}-{dtype}-P33-sh{shrink}", "retire", preset, dtype, 33, (6, 3, 11), options=(("shrink", shrink),),
                            census=(("rows_attn", True),), steps=10, ends=(1, 10, 10)))
    # best-of-N: slots u * N + j; the siblings j > 0 get copies of [P, ...) of their text's first sample
    for preset, dtype, P in (("tiny128", "bf16", 33), ("tiny_h16", "bf16", 64), ("tiny128", "fp32", 64), ("tiny", "fp32", 33)):
        out.append(Case(f"bestof-{preset}-{dtype}-P{P}", "best_of", preset, dtype, P, (5, 9), N=2, census=(("rows_attn", True),)))
    return out


CASES = _prefill_cases() + _decode_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def model(preset):
    from voicecraft_amd import synth
    a = synth.make_args(preset)
    return a, synth.make_state_dict(a, seed=SEED)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """texts / stale texts (lists of int64 [Lx]), y / stale y (int64 [T, K]), forced tokens int64 [n, slots, K] of a case."""
    c = BY_NAME[name]
    a, _ = model(c.preset)
    rs = np.random.RandomState(zlib.crc32(name.encode()))
    V, K = a.text_vocab_size, a.n_codebooks
    prefix = rs.randint(0, V, size=c.P)
    first = rs.permutation(V)[: c.B]                      # the texts differ AT index P
    texts = []
    for u, n in enumerate(c.lens):
        sent = rs.randint(0, V, size=n)
        sent[0] = first[u]
        texts.append(np.concatenate([prefix, sent]).astype(np.int64))
    stale = [((t + 1 + rs.randint(0, V - 1, size=t.shape)) % V).astype(np.int64) for t in texts]      # differs at EVERY index
    y = rs.randint(0, a.audio_vocab_size, size=(c.T, K)).astype(np.int64)
    y_stale = rs.randint(0, a.audio_vocab_size, size=(c.T, K)).astype(np.int64)
    n = max(c.end(s) for s in range(c.slots)) + K
    forced = np.zeros((n, c.slots, K), dtype=np.int64)
    for s in range(c.slots):
        e = c.end(s)
        forced[:e, s] = rs.randint(0, a.audio_vocab_size, size=(e, K))
        for j in range(K):                    # the staggered end of the span (voicecraft.py:1057-1066): the slot ends with its forced steps
            forced[e + j, s, :j] = a.empty_token
            forced[e + j, s, j] = a.eos
    as_t = lambda v: [torch.from_numpy(t) for t in v]
    return as_t(texts), as_t(stale), torch.from_numpy(y), torch.from_numpy(y_stale), forced


# ------------------------------------------------------------------------------------------------ the reference's defect models
class PrefixOracle(VoiceCraftOracle):
    """VoiceCraftOracle whose attention (a) records the prefill's K/V per layer in `self.rec` and (b) replaces, whenever K/V are read,
    the rows of `self.subst` = [(position, donor)] by the rows a donor run recorded (`rec` of another PrefixOracle call).  The cache
    itself keeps the run's own rows, as the engine's does: only the READ is redirected."""

    def __init__(self, args, state_dict):
        super().__init__(args, state_dict)
        self.rec: dict = {}
        self.subst: list = []

    def _attn(self, l, x, mask, past_l):
        p = f"decoder.layers.{l}.self_attn."
        B, n, d = x.shape
        H, hd = self.H, self.hd
        xt = x.transpose(1, 0)
        proj = F.linear(xt, self.sd[p + "in_proj_weight"], self.sd[p + "in_proj_bias"])
        proj = proj.unflatten(-1, (3, d)).unsqueeze(0).transpose(0, -2).squeeze(-2).contiguous()
        q, k, v = proj[0], proj[1], proj[2]
        q = q.view(n, B * H, hd).transpose(0, 1).view(B, H, n, hd)
        k = k.view(n, B * H, hd).transpose(0, 1).view(B, H, n, hd)
        v = v.view(n, B * H, hd).transpose(0, 1).view(B, H, n, hd)
        present = torch.stack([k, v], dim=0)
        if past_l is not None:
            k = torch.cat([past_l[0], k], dim=-2)
            v = torch.cat([past_l[1], v], dim=-2)
        else:
            self.rec[l] = (k.clone(), v.clone())
        if self.subst:
            k, v = k.clone(), v.clone()
            for pos, donor in self.subst:
                k[:, :, pos] = donor[l][0][:, :, pos]
                v[:, :, pos] = donor[l][1][:, :, pos]
        o = F.scaled_dot_product_attention(q, k, v, mask, 0.0, is_causal=False)
        o = o.permute(2, 0, 1, 3).contiguous().view(B * n, d)
        o = F.linear(o, self.sd[p + "out_proj.weight"], self.sd[p + "out_proj.bias"]).view(n, B, d)
        return o.transpose(1, 0), present

    def run(self, x, y, forced, steps, subst=()):
        """Teacher-forced head logits [steps, K, V] of inference_tts on text x [Lx], audio prompt y [T, K]; returns (logits, rec)."""
        self.rec, self.subst = {}, list(subst)
        trace = []
        self.inference_tts(x.unsqueeze(0), torch.tensor([x.numel()]), y.unsqueeze(0), top_k=1, stop_repetition=3, trace=trace,
                           forced=forced, max_steps=steps)
        self.subst = []
        return torch.stack([t["logits"][0] for t in trace[:steps]]).numpy(), self.rec


@functools.lru_cache(maxsize=None)
def reference(name):
    """From the oracle alone: {"clean": per slot the clean logits [n_steps(slot), K, V], "models": {(model, slot): smallest rel L2 over
    the slot's steps}, "floor": the smallest of them}.  The GPU tests and the CPU test call this same function; the arrays are shared
    and must not be written."""
    c = BY_NAME[name]
    a, sd = model(c.preset)
    K = a.n_codebooks
    texts, stale, y, y_stale, forced = inputs(name)
    orc = PrefixOracle(a, sd)
    clean, rec = {}, {}
    for s in range(c.slots):
        clean[s], r = orc.run(texts[s // c.N], y, forced[:, s], c.n_steps(s, K))
        if s % c.N == 0:
            rec[s // c.N] = r
        clean[s].setflags(write=False)
    rec_stale = {u: orc.run(stale[u], y_stale, forced[:, u * c.N], 1)[1] for u in range(c.B)}
    models = {}
    for s in range(1, c.slots):
        u, j = divmod(s, c.N)
        todo = {"M2": (c.P - 1, rec_stale[u])}
        if u > 0:
            todo["M1"] = (c.P, rec[0])
        if j > 0:
            todo["M3"] = (c.P, rec_stale[u])
        for m, sub in todo.items():
            got, _ = orc.run(texts[u], y, forced[:, s], c.n_steps(s, K), subst=[sub])
            models[(m, s)] = float(rel_l2(got, clean[s]).min())
    return {"clean": clean, "models": models, "floor": min(models.values())}


def defect_floor(case):
    """Case or case name -> the floor (memoised in `reference`)."""
    return reference(getattr(case, "name", case))["floor"]
