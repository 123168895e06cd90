"""Prefill attention (tile_attn_k, tile_attn64_k; voicecraft_amd/csrc/vc_attn.hip) against float64: the launches of
tests/test_gpu_prefill_attn.py, their inputs, the reference, the bars and the defect models.  No GPU in this module.

One LAUNCH is a prefill pass's row stream (check_layout restates the rule of prefill_batch): prompts back to back, each starting on a
multiple of 16 rows (tile_attn64_k: 64), a prompt's rows at consecutive positions p0 .. p0 + n - 1 of ONE sequence slot, padding rows
(row_pos = -1, row_seq = 0 as the engine leaves them) only behind a prompt's last row.  p0 = 0 for a first pass, a multiple of the
alignment for a continuation pass (the cache below p0 holds data), `share` for the sequences other than 0 of a shared-prefix call
(positions below `share` are read from sequence 0).  The slots are a rotation, so seq != prompt index, and one slot is unused.

What the kernel is handed (kernel_caches): K and V of positions 0..last of each sequence and sequence 0's prefix are finite; every
position above a sequence's last one, every position below `share` in a sequence other than 0 (own_prefix = False) and the unused
slot are NaN.  With own_prefix = True the other sequences hold FOREIGN finite numbers below `share`.  q is finite in every row.

Inputs are bf16-exact, so one float64 reference serves both dtypes.  The bf16 kernels hand the MFMA bf16(q * scale * log2 e); the
reference does not restate that rounding: the log2-unit vector qhat is generated bf16-exact, the kernel gets q = fp32(qhat / qs)
with qs the kernel's own fp32 product scale * log2 e, and tests/test_prefill_attn_cpu.py checks that fp32 q * qs rounds back to
qhat.  reference = softmax2(qhat . K) V in float64 over the visible positions; it knows nothing of tiles, waves or stages.

Families
  flat     as the decode suite's: scores within +-0.25, |V| in [0.5, 1.5] with random signs.  Every (row, position) pair is covered.
  uniform  all K rows of a launch's head are identical (per sequence when no prefix is shared), so every visible score of a row is
           the same number whatever the summation order and every probability is exp2(0) = 1; V holds integers in [-128, 128]:
           every product and sum before the final division is exact in both dtypes.  Every (row, position) pair is covered.
  probe    the flat inputs with at most 16 positions per sequence lifted by about +6 in score (natural units; K rows that are
           multiples of the sequence's one qhat): 0, share - 1, share, last, both sides of key-tile boundaries and positions whose
           residues modulo the key-tile width, over the variants of a case set, are all of them.  A lifted p is seen by every row at
           or behind it, and must not be seen by row p - 1.
  peaked   raw scores from -120 to +60 with a run of five EQUAL maxima of +100 placed across a key-tile boundary, rows on either
           side of and inside the run.  The rows of a prompt share their K, so position 0 holds the same maximum: every row, also
           one in front of the run, is then governed by equal maxima as every row of the decode suite's family is - two DISTINCT
           scores near 100 differ by several fp32 ulps of 100 in any fp32 score product, which is more than the fp32 bar allows.

Bars (per element, derived; `bars`)
  fp32 forms                      2^-18 max|V|   (decode_attn_cases.BAR32)
  bf16 forms, flat/probe/peaked   2^-7 sum_p w_p |V_pj| + 2^-18 max|V|: one 2^-8 rounding of every probability (the kernels sum the
                                  unrounded ones) and one of the stored output
  bf16 forms, uniform             2^-8 |ref_j| + 2^-18 max|V|: only the output rounding remains

Defect models, applied to the reference at every covered position p of every row that sees it: p dropped; p counted twice; p replaced
by its neighbour; pos + 1 included; p < share taken from the row's own sequence.  A launch is admitted if every model moves some
element by at least SENS_MIN = 8 bars - at EVERY covered (row, position) pair of the dense families (flat, uniform), in SOME row
that sees it for every lifted position of the sparse ones (tests/test_prefill_attn_cpu.py)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import decode_attn_cases as dc

H = dc.H
NW = 4                                   # waves of a tile_attn_k workgroup
SENS_MIN = dc.SENS_MIN
BAR32 = dc.BAR32
BAR16_P = 2.0 ** -7                      # bf16 forms: probabilities and output rounded
BAR16_OUT = 2.0 ** -8                    # bf16 forms, uniform family: the output rounding alone
LIFT2 = dc.LIFT * np.log2(np.e)          # probe family: score of a lifted position, in log2 units
N_PROBES = dc.N_PROBES
PREFIX_PROBES = dc.PREFIX_PROBES
PEAK2, PEAK_LOW2, PEAK_HIGH2 = (x * np.log2(np.e) for x in (dc.PEAK, dc.PEAK_LOW, dc.PEAK_HIGH))
RUN = dc.RUN
MAX_ROWS = 704
FORMS = tuple((1, dtype, hd) for dtype in dc.DTYPES for hd in dc.HDS) + ((2, "bf16", 128),)
DENSE = ("flat", "uniform")


def kw(form, dtype):
    """Keys of one key tile."""
    return 64 if form == 2 else 32 if dtype == "bf16" else 16


def align(form):
    """Rows of one workgroup: prompts start on multiples of it."""
    return 64 if form == 2 else 16


def qs(hd):
    """The factor the kernels apply to q: fp32 scale * fp32 log2 e, an fp32 product."""
    return float(np.float32(dc.kernel_scale(hd)) * np.float32(1.4426950408889634))


def families(form, dtype, kind):
    """The families a launch kind is listed in for a form.  flat does not separate one position from a bf16 rounding beyond S of
    about 17 and is listed for the bf16 forms only in the `short` launches; peaked has no shared-prefix launches."""
    f = ["uniform", "probe"]
    if kind != "share":
        f.append("peaked")
    if dtype == "fp32" or kind == "short":
        f.append("flat")
    return tuple(f)


# ------------------------------------------------------------------------------------------------ the key partition, restated
def key_tiles(form, dtype, pos0, na, wave):
    """First keys of the key tiles wave `wave` visits, and the last key it may read.  Form 1: the workgroup's row tile starts at position
    pos0 with na active rows; waves w, w + NW, ... take key tiles of KW keys.  Form 2: pos0 / na are the 64-row BLOCK's, wave w owns
    its rows 16 w .. 16 w + 15 and takes the 64-key tiles in order up to the one holding its last row's position."""
    KW = kw(form, dtype)
    if form == 1:
        last = pos0 + na - 1
        return list(range(wave * KW, last + 1, NW * KW)), last
    na_w = max(0, min(16, na - 16 * wave))
    t_last = pos0 + 16 * wave + na_w - 1
    if na_w == 0:
        return [], t_last
    return [kt0 for kt0 in range(0, pos0 + na, KW) if kt0 <= t_last], t_last


# ------------------------------------------------------------------------------------------------ launches
@dataclass
class Launch:
    form: int
    dtype: str
    hd: int
    family: str
    kind: str
    share: int
    prompts: list             # (seq, p0, n, row0) in row order
    n_slots: int
    qhat: np.ndarray          # fp32 [rows][H * hd], bf16-exact: the log2-unit query vectors
    Kf: np.ndarray            # fp32 [n_slots][H][S_max + 1][hd], no NaN: what the slots would hold if they went on (defect models)
    Vf: np.ndarray
    row_seq: np.ndarray       # int32 [rows]
    row_pos: np.ndarray
    covered: dict = field(default_factory=dict)      # sparse families: seq -> sorted positions the defect models are applied at
    tag: str = ""

    @property
    def rows(self):
        return len(self.row_pos)

    @property
    def S_max(self):
        return self.Kf.shape[2] - 1

    @property
    def q(self):
        """What the kernel is handed: fp32(qhat / qs)."""
        return (self.qhat.astype(np.float64) / qs(self.hd)).astype(np.float32)

    @property
    def name(self):
        return f"{self.kind}{self.tag}-{self.family}-f{self.form}-{self.dtype}-hd{self.hd}-sh{self.share}"


def check_layout(L):
    """prefill_batch's rule, restated."""
    al = align(L.form)
    assert L.rows % al == 0 and 0 < L.rows <= MAX_ROWS
    seqs = [p[0] for p in L.prompts]
    assert len(set(seqs)) == len(seqs) and all(0 <= s < L.n_slots for s in seqs) and len(seqs) < L.n_slots      # ... one slot unused
    assert all(s != i for i, s in enumerate(seqs)), "seq is a rotation of the slots"
    assert 0 <= L.share <= L.S_max
    row = 0
    for seq, p0, n, row0 in L.prompts:
        assert row0 == row and row0 % al == 0 and n >= 1 and p0 + n <= L.S_max
        assert (L.row_seq[row0:row0 + n] == seq).all() and (L.row_pos[row0:row0 + n] == p0 + np.arange(n)).all()
        row = row0 + (n + al - 1) // al * al
        assert (L.row_pos[row0 + n:row] == -1).all() and (L.row_seq[row0 + n:row] == 0).all()      # padding only behind the last row
        if L.share and seq != 0:
            assert p0 == L.share
        else:
            assert p0 % al == 0          # 0: a first pass; a multiple of the alignment: a continuation pass
    assert row == L.rows
    if L.share:
        s0 = [p for p in L.prompts if p[0] == 0]
        assert s0 and s0[0][1] == 0 and s0[0][2] >= L.share, "sequence 0 holds the prefix rows"
    assert np.isfinite(L.q).all() and np.isfinite(L.Kf).all() and np.isfinite(L.Vf).all()


def _along(qh, score):
    """K rows [len(score)][hd] whose log2-unit score against qh is about `score` each: multiples of qh, rounded to bf16."""
    c = np.asarray(score, dtype=np.float64) / float(qh.astype(np.float64) @ qh.astype(np.float64))
    return dc.bf16_exact(c[:, None] * qh[None, :].astype(np.float64))


@functools.lru_cache(maxsize=8)
def content(hd, n_pos):
    """The decode suite's flat numbers with K rescaled (by a power of two) for LOG2-unit scores within +-0.25 against q used as qhat."""
    cq, cK, cV = dc.content(hd, n_pos)
    sc = np.einsum("qhd,chsd->qchs", cq.astype(np.float64), cK.astype(np.float64))
    K = cK * np.float32(2.0 ** np.floor(np.log2(0.25 / np.abs(sc).max())))
    K.setflags(write=False)
    return cq, K, cV


def _pick_lifted(KW, lo, hi, diag_lo, musts, budget, variant, nvar):
    """At most `budget` positions of [lo, hi]: `musts`, both sides of the key-tile boundaries (every nvar-th pair, starting at pair
    `variant`), then positions at or behind diag_lo (rows of the launch sit on their diagonal) whose residues modulo KW walk with the
    variant."""
    pos = sorted({int(p) for p in musts if lo <= p <= hi})
    if hi - lo + 1 <= budget:
        return list(range(lo, hi + 1))
    pairs = [(b - 1, b) for b in range(KW, hi + 1, KW) if b - 1 >= lo]
    room = max(0, (budget - len(pos)) // 2)
    take = pairs[variant % nvar::nvar][:max(room - 1, min(room, 1))] if pairs else []
    for a, b in take:
        pos += [p for p in (a, b) if p not in pos]
    fill = budget - len(pos)
    d0 = max(diag_lo, lo)
    for i in range(fill):
        r = (variant * -(-KW // nvar) + i) % KW
        cand = [p for p in range(d0 + (r - d0) % KW, hi + 1, KW) if p not in pos]
        if cand:
            pos.append(cand[(5 * i + variant) % len(cand)])
    return sorted(pos)[:budget]


def make_launch(form, dtype, hd, family, kind, lens, share=0, variant=0, nvar=4, tag=""):
    """lens: [(n, p0)] per prompt in row order.  Without a shared prefix prompt i sits in slot (i + 1) % (prompts + 1) and slot 0 is the
    unused one; with one, in slot (i + 1) % prompts - the LAST prompt is sequence 0's - and the unused slot is the last."""
    al, KW = align(form), kw(form, dtype)
    n_pr = len(lens)
    assert family in ("flat", "uniform", "probe", "peaked") and (share == 0 or n_pr >= 2)
    n_slots = n_pr + 1
    seqs = [(i + 1) % (n_pr if share else n_slots) for i in range(n_pr)]
    prompts, row = [], 0
    for (n, p0), s in zip(lens, seqs):
        prompts.append((s, int(p0), int(n), row))
        row += (n + al - 1) // al * al
    rows = row
    S_max = max(p0 + n for n, p0 in lens)
    cq, cK, cV = content(hd, S_max + 1)
    rng = np.random.RandomState(131 * hd + 17 * share + 7 * variant + len(family) + rows)
    row_seq, row_pos = np.zeros(rows, dtype=np.int32), np.full(rows, -1, dtype=np.int32)
    for s, p0, n, r0 in prompts:
        row_seq[r0:r0 + n], row_pos[r0:r0 + n] = s, p0 + np.arange(n)
    Kf = np.stack([cK[0 if s == 0 else 1] for s in range(n_slots)]).copy()
    Vf = np.stack([cV[0 if s == 0 else 1] for s in range(n_slots)]).copy()
    qi = np.arange(rows) % dc.NQ                       # flat, uniform: the q vectors cycle over the rows (padding rows hold one too)
    covered = {}
    if family == "uniform":
        krow = dc.bf16_exact(rng.uniform(-0.5, 0.5, (n_slots, H, hd)))
        if share:
            krow[:] = krow[0]                          # rows behind a prefix read two slots: one K row for the launch
        Kf[:] = krow[:, :, None, :]
        Vf = rng.randint(-128, 129, size=Vf.shape).astype(np.float32)
    elif family in ("probe", "peaked"):
        for s, p0, n, r0 in prompts:
            qi[r0:r0 + (n + al - 1) // al * al] = 0 if share else s % dc.NQ       # one qhat per sequence; per launch behind a prefix
        prefix = _pick_lifted(KW, 0, share - 1, 0, {0, share - 1}, PREFIX_PROBES, variant, nvar) if share else []
        for i, (s, p0, n, r0) in enumerate(prompts):
            last = p0 + n - 1
            qv = cq[qi[r0]]
            if family == "probe":
                if share:
                    own = _pick_lifted(KW, share, last, share, {share, last}, N_PROBES - PREFIX_PROBES, variant + i, nvar) if last >= share else []
                    pos = sorted(set(prefix) | set(own))
                else:
                    pos = _pick_lifted(KW, 0, last, p0, {0, p0, last}, N_PROBES, variant + i, nvar)
                for h in range(H):
                    for p, kr in zip(pos, _along(qv[h], np.full(len(pos), LIFT2))):
                        Kf[0 if p < share else s, h, p] = kr
            else:
                assert share == 0
                bs = [b for b in range(KW, last + 1, KW) if b - 2 >= max(p0, 0) and b + 2 <= last]
                b0 = bs[(variant + i) % len(bs)] - 2 if bs else max(0, last - RUN + 1)
                pos = sorted({0} | set(range(b0, min(b0 + RUN, last + 1))))          # position 0: every row is governed by EQUAL maxima
                target = rng.uniform(PEAK_LOW2, PEAK_HIGH2, S_max + 1)
                target[pos] = PEAK2
                for h in range(H):
                    Kf[s, h] = _along(qv[h], target)
            covered[s] = np.array(pos, dtype=np.int64)
    qhat = np.stack([cq[j].reshape(H * hd) for j in qi])
    return Launch(form, dtype, hd, family, kind, int(share), prompts, n_slots, qhat, Kf, Vf, row_seq, row_pos, covered, tag)


def kernel_caches(L, own_prefix=False):
    """K / V as the kernel gets them: fp32 [n_slots][H][S_max][hd] (module docstring)."""
    K = np.full(L.Kf[:, :, : L.S_max].shape, np.nan, dtype=np.float32)
    V = K.copy()
    for s, p0, n, r0 in L.prompts:
        lo = L.share if (s != 0 and not own_prefix) else 0
        K[s, :, lo:p0 + n], V[s, :, lo:p0 + n] = L.Kf[s, :, lo:p0 + n], L.Vf[s, :, lo:p0 + n]
    return K, V


# ------------------------------------------------------------------------------------------------ reference and bars
def prompt_eval(L, K, V, pi):
    """softmax2(qhat . K) V of one prompt's rows in float64, out of caches K / V: weights e [H][n][S] (0 where the row does not see the
    position), their sums D [H][n], out / wabs (sum_p w_p |V_p|) [H][n][hd], vmax [H][n] (largest |V| the row sees)."""
    s, p0, n, r0 = L.prompts[pi]
    hd, S = L.hd, p0 + n
    sh = min(L.share, S) if s else 0
    Kr = np.concatenate([K[0, :, :sh], K[s, :, sh:S]], axis=1).astype(np.float64)
    Vr = np.concatenate([V[0, :, :sh], V[s, :, sh:S]], axis=1).astype(np.float64)
    qh = L.qhat[r0:r0 + n].reshape(n, H, hd).astype(np.float64)
    sc = np.einsum("nhd,hsd->hns", qh, Kr)
    pos = p0 + np.arange(n)
    vis = np.arange(S)[None, :] <= pos[:, None]
    sc = np.where(vis[None], sc, -np.inf)
    m = sc.max(axis=-1)
    e = np.exp2(sc - m[..., None])
    D = e.sum(axis=-1)
    N = np.einsum("hns,hsd->hnd", e, Vr)
    out = N / D[..., None]
    wabs = np.einsum("hns,hsd->hnd", e, np.abs(Vr)) / D[..., None]
    vmax = np.maximum.accumulate(np.abs(Vr).max(axis=-1), axis=-1)[:, p0:S]
    return dict(qh=qh, Kr=Kr, Vr=Vr, pos=pos, vis=vis, m=m, e=e, D=D, out=out, wabs=wabs, vmax=vmax)


def bars(ev, family):
    """(fp32-form bar, bf16-form bar), [H][n][hd] each (module docstring)."""
    b32 = BAR32 * ev["vmax"][..., None] * np.ones_like(ev["out"])
    b16 = b32 + (BAR16_OUT * np.abs(ev["out"]) if family == "uniform" else BAR16_P * ev["wabs"])
    return b32, b16


def _flat_rows(x):
    """[H][n][hd] -> [n][H * hd]"""
    return x.transpose(1, 0, 2).reshape(x.shape[1], -1)


def reference(L, K=None, V=None):
    """(out, bar32, bar16), [rows][H * hd] float64 each, from the caches the kernel is handed; padding rows: zeros, and bars of zero."""
    if K is None:
        K, V = kernel_caches(L)
    out, b32, b16 = (np.zeros((L.rows, H * L.hd)) for _ in range(3))
    for pi, (s, p0, n, r0) in enumerate(L.prompts):
        ev = prompt_eval(L, K, V, pi)
        assert np.isfinite(ev["Kr"]).all() and np.isfinite(ev["Vr"]).all()
        a, b = bars(ev, L.family)
        out[r0:r0 + n], b32[r0:r0 + n], b16[r0:r0 + n] = _flat_rows(ev["out"]), _flat_rows(a), _flat_rows(b)
    return out, b32, b16


# ------------------------------------------------------------------------------------------------ defect models
def _reduce(ratio, ok, dense):
    """ratio / ok [n][C] -> the launch figure: the smallest over every covered pair (dense), or over the columns of the largest over
    the rows that see the column (sparse).  None where nothing applies."""
    if not ok.any():
        return None
    if dense:
        return float(ratio[ok].min())
    col = np.where(ok & ~np.isnan(ratio), ratio, -np.inf).max(axis=0)          # (0 / 0: a row whose other weights vanish beside p's)
    return float(col[ok.any(axis=0)].min())


def prompt_sensitivity(L, K, V, pi, chunk=32):
    """{model: smallest defect / bar} of one prompt against the bar of the launch's dtype.  A model that does not apply is left out."""
    s, p0, n, r0 = L.prompts[pi]
    dense = L.family in DENSE
    ev = prompt_eval(L, K, V, pi)
    S = p0 + n
    bar = bars(ev, L.family)[0 if L.dtype == "fp32" else 1]
    cols = np.arange(S) if dense else np.array([p for p in L.covered[s] if p < S], dtype=np.int64)
    Vr, e, D, out, pos, qh, m = ev["Vr"], ev["e"], ev["D"], ev["out"], ev["pos"], ev["qh"], ev["m"]
    R = {k: np.zeros((n, len(cols))) for k in ("drop", "twice", "neighbour")}
    below = cols < L.share if s else np.zeros(len(cols), dtype=bool)
    if below.any():
        R["own_prefix"] = np.zeros((n, int(below.sum())))
        Ko, Vo = L.Kf[s][:, cols[below]].astype(np.float64), L.Vf[s][:, cols[below]].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            ib = 1.0 / bar[:, c0:c1, None, :]
            oc, Dc = out[:, c0:c1, None, :], D[:, c0:c1, None]
            ep = e[:, c0:c1][:, :, cols]
            Gv = Vr[:, None, cols, :] - oc
            nb = np.clip(np.where(cols[None, :] < pos[c0:c1, None], cols[None, :] + 1, cols[None, :] - 1), 0, S - 1)
            enb = np.take_along_axis(e[:, c0:c1], nb[None], axis=2)
            Gn = Vr[:, nb, :] - oc
            mx = lambda d: (np.abs(d) * ib).max(axis=(0, 3))
            R["drop"][c0:c1] = mx((ep / (Dc - ep))[..., None] * Gv)
            R["twice"][c0:c1] = mx((ep / (Dc + ep))[..., None] * Gv)
            R["neighbour"][c0:c1] = mx((enb[..., None] * Gn - ep[..., None] * Gv) / (Dc - ep + enb)[..., None])
            if below.any():
                eo = np.exp2(np.einsum("nhd,hcd->hnc", qh[c0:c1], Ko) - m[:, c0:c1, None])
                epb = ep[:, :, below]
                R["own_prefix"][c0:c1] = mx((eo[..., None] * (Vo[:, None] - oc) - epb[..., None] * Gv[:, :, below]) / (Dc - epb + eo)[..., None])
    see = (cols[None, :] <= pos[:, None]) & (pos[:, None] >= 1)          # a row of one position is its V whatever its weight
    res = {k: _reduce(R[k], see if k != "own_prefix" else np.ones_like(R[k], dtype=bool), dense) for k in R}
    # pos + 1 included: read where the kernel would read it
    sx = np.where(pos + 1 < L.share, 0, s)
    Kx, Vx = L.Kf[sx, :, pos + 1].astype(np.float64), L.Vf[sx, :, pos + 1].astype(np.float64)          # [n][H][hd]
    ex = np.exp2(np.einsum("nhd,nhd->hn", qh, Kx) - m)
    d = ex[..., None] * (Vx.transpose(1, 0, 2) - out) / (D + ex)[..., None]
    rb = (np.abs(d) / bar).max(axis=(0, 2))
    okb = np.ones(n, dtype=bool) if dense else np.isin(pos + 1, L.covered[s])
    res["beyond"] = float(rb[okb].min()) if okb.any() else None
    return {k: v for k, v in res.items() if v is not None}


def launch_sensitivity(L):
    """{model: smallest defect / bar}, the minimum over the launch's prompts."""
    K, V = kernel_caches(L)
    res = {}
    for pi in range(len(L.prompts)):
        for k, v in prompt_sensitivity(L, K, V, pi).items():
            res[k] = min(v, res.get(k, np.inf))
    return res


# ------------------------------------------------------------------------------------------------ the tables
def sweep_rows(form):
    return 384 if form == 2 else 320


def sweep_variants(form, dtype, family):
    """Probe launches of one case set whose lifted diagonals take every residue modulo the key-tile width."""
    return (6 if form == 2 else 4) if family == "probe" else 1


def sweep_launches(form, dtype, hd):
    """Every length at once: one sequence of 320 (form 2: 384) rows from position 0, in every family listed for the form."""
    out = []
    for f in families(form, dtype, "sweep"):
        nv = sweep_variants(form, dtype, f)
        out += [make_launch(form, dtype, hd, f, "sweep", [(sweep_rows(form), 0)], variant=v, nvar=nv, tag=str(v)) for v in range(nv)]
    return out


RAGGED = {1: [(33, 0), (47, 0), (48, 0), (5, 0), (100, 0)],          # last tiles of 1, 15, 16 and 5 rows; a prompt shorter than a key tile
          2: [(1, 0), (16, 0), (81, 0), (127, 0), (128, 0)]}         # last blocks of 1, 16, 17, 63 and 64 rows
SHORT = {1: [(16, 0), (3, 0), (9, 0), (15, 0)], 2: [(16, 0), (3, 0), (9, 0)]}
CONT = {1: [(40, 16), (37, 128), (50, 144)], 2: [(70, 64), (100, 192)]}


def ragged_launches(form, dtype, hd):
    """Prompts side by side, blocks of different sequences adjacent; and the `short` stream (every prompt within one 16-row tile), the
    only launches the flat family is listed in for the bf16 forms."""
    return ([make_launch(form, dtype, hd, f, "ragged", RAGGED[form], variant=1) for f in families(form, dtype, "ragged")] +
            [make_launch(form, dtype, hd, f, "short", SHORT[form], variant=2) for f in families(form, dtype, "short")])


def cont_launches(form, dtype, hd):
    """Continuation passes: p0 = 16, 128, 144 (form 2: 64, 192), the earlier positions present only in the cache."""
    return [make_launch(form, dtype, hd, f, "cont", CONT[form], variant=3) for f in families(form, dtype, "cont")]


def share_values(form, dtype):
    """[(share, rows of sequence 0 behind the prefix)]: 1, KW - 1, KW, KW + 1, NW KW +- 1, 16 k + 5 and a value inside the last key
    tile; form 2: 1, 63, 64, 65, 127..129, 64 k + 37, and 62.  The value inside the last key tile (and form 2's 62) is KW - 2 modulo
    KW: the other sequences' row tiles then start ONE position in front of a key tile's last key, where the switch between the
    mask-free and the masked softmax (kt0 + KW - 1 <= pos0) is decided by one position."""
    KW = kw(form, dtype)
    if form == 2:
        return [(1, 70), (62, 20), (63, 20), (64, 20), (65, 20), (127, 20), (128, 20), (129, 3), (165, 40)]
    return [(1, 40), (KW - 1, 20), (KW, 20), (KW + 1, 20), (NW * KW - 1, 20), (NW * KW + 1, 20), (16 * 3 + 5 + (KW == 16) * 32, 30),
            (6 * KW - 2, 1)]


def share_launches(form, dtype, hd):
    """Sequence 0 holds the prefix rows and a few behind them; two others start at p0 = share, so their tile positions are unaligned."""
    other = (70, 21) if form == 2 else (21, 40)
    out = []
    for i, (sh, tail) in enumerate(share_values(form, dtype)):
        lens = [(n, sh) for n in other] + [(sh + tail, 0)]
        out += [make_launch(form, dtype, hd, f, "share", lens, share=sh, variant=i) for f in families(form, dtype, "share")]
    return out


def all_launches(form, dtype, hd):
    return sweep_launches(form, dtype, hd) + ragged_launches(form, dtype, hd) + cont_launches(form, dtype, hd) + share_launches(form, dtype, hd)
