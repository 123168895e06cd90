"""Decode attention (rows_attn_k, voicecraft_amd/csrc/vc_attn.hip) against float64: the case table of tests/test_gpu_decode_attn.py,
its inputs, the reference, the host-side merge of split partials, the bars and the defect models.  No GPU in this module.

One LAUNCH is a set of rows, each at its own (sequence, position): row r attends to positions 0..pos of sequence seq[r], positions
below `share` coming from sequence 0.  seq is a rotation of the slots, so seq != row.  Every input is bf16-exact: the fp32 and the
bf16 kernel read the same numbers, and one float64 reference serves both.

The kernel's arithmetic of positions (restated by chunk_rule / splits): a row of S = pos + 1 positions is cut into nsplit chunks of
`chunk` positions; a workgroup of NW = 8 waves visits its chunk in batches of BATCH = 4 * 8 * PPW positions (PPW = positions a wave
reads per request: 64 lanes / (head_dim / elements per 16-byte load)); the first batch is addressed one way when no prefix is shared,
every later batch ("refill") and every batch of a shared-prefix call another way.  Only the MERGED row is the contract: the reference
knows nothing of the partition.

Families
  flat    scores within +-0.25, |V| in [0.5, 1.5] with random signs: every position carries about 1 / S of the row.
  probe   the flat inputs with up to 16 positions per row lifted by about +6 in score (their K rows are a multiple of the row's q):
          the first and last position of every split's chunk, 0, pos, share - 1, share, both sides of every batch boundary inside
          a chunk (sampled down to 16 where there are more).  Each lifted position holds a few per cent of the row even at S = 4000;
          only the lifted positions count as covered.  With a shared prefix all rows of a launch use one q, ten of the lifted
          positions lie below `share` (0, share - 1, edges of the longest row's chunks) and are common to the rows, six are the
          row's own (share, pos, its chunk edges behind the prefix).
  peaked  raw scores between -120 and +100 (beyond the +-88 at which a bare fp32 exponential overflows), one run of up to five EQUAL
          maxima; the run is what counts as covered.

What the kernel is handed (kernel_caches): every position above a sequence's own pos is NaN, and so is every position below `share`
in a sequence other than 0 - a causal leak or a read on the wrong side of the prefix boundary shows as NaN, not as a small number.

Bars (derived, per element; `bars`)
  fp32 outputs (fp32 partials of either cache dtype, fp32 x_out):  2^-18 * max|V| - 64 fp32 ulps of the largest value, for sums of S
          terms in another order and a hardware exp2 of 1 ulp.
  bf16 outputs (bf16 partials, bf16 x_out):  that + 2^-8 * sum_p w_p |V_pj| with w the reference weights - one bf16 rounding
          (8 significant bits: at most 2^-8 relative, reached just above a power of two) of each partial under ANY partition, since
          the partials' magnitudes add up to at most that sum.  A correct kernel can therefore come close to this bar.

Defect models (row_sensitivity), applied to the float64 reference at every covered position p: p dropped; p counted twice; p
replaced by its neighbour; pos + 1 included; p < share taken from the row's own sequence.  A case is admitted only if every model
moves some element of the merged row by at least SENS_MIN = 8 times that element's bar (tests/test_decode_attn_cpu.py)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch

H = 2                     # heads of every launch
NW = 8                    # waves per workgroup (VC_ATT_WAVES)
EPL = {"fp32": 4, "bf16": 8}          # cache elements per 16-byte load
DTYPES = ("fp32", "bf16")
HDS = (32, 64, 128)
MAX_NSPLIT = 8
EDGE_NSPLITS = (1, 2, 3, 5, 7, 8)
NQ = 4                    # distinct q vectors, cycled over the rows
LIFT = 6.0                # probe family: score of a lifted position
N_PROBES = 16
PREFIX_PROBES = 10        # probe family with a shared prefix: lifted positions below `share`, common to the rows of the launch
PEAK, PEAK_LOW, PEAK_HIGH, RUN = 100.0, -120.0, 60.0, 5
SENS_MIN = 8.0
BAR32 = 2.0 ** -18
BAR16 = 2.0 ** -8


def ppw(dtype, hd):
    return 64 * EPL[dtype] // hd


def batch(dtype, hd):
    return 4 * NW * ppw(dtype, hd)


def sweep_top(dtype, hd):
    """One past the first refill of an 8-way split, and 64 more."""
    return MAX_NSPLIT * batch(dtype, hd) + 65


def kernel_scale(hd):
    """1 / sqrt(hd) as the launcher computes it (fp32)."""
    return float(np.float32(1.0) / np.sqrt(np.float32(hd)))


def bf16_exact(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


# ------------------------------------------------------------------------------------------------ the partition
def chunk_rule(S, n):
    """The kernel's chunk length in numpy float32: (int)((float)(S + n - 1) * nextafter(1 / n, 2)), + 1 if chunk * n < S."""
    S = np.asarray(S, dtype=np.int64)
    inv = np.nextafter(np.float32(1.0) / np.float32(n), np.float32(2.0))
    c = ((S + (n - 1)).astype(np.float32) * inv).astype(np.int64)
    return c + (c * n < S)


def splits(S, n):
    """[(p0, p1)] of the n splits of a row of S positions (p0 >= p1: an empty split)."""
    c = int(chunk_rule(S, n))
    return [(i * c, min(S, i * c + c)) for i in range(n)]


def empty_last_split(n):
    """The smallest S > n whose last split is empty (9 with n = 8); None where there is none (n <= 2)."""
    for S in range(n + 1, 65):
        p0, p1 = splits(S, n)[-1]
        if p0 >= p1:
            return S
    return None


def edge_lengths(dtype, hd, n):
    """The context lengths of an edge launch; the largest of them is the launch's S_max."""
    P, B = ppw(dtype, hd), batch(dtype, hd)
    s = {1, 2, n - 1, n, n + 1, P - 1, P + 1, 8 * P - 1, 8 * P + 1, B - 1, B, B + 1, n * B - 1, n * B, n * B + 1, 2 * B + 1}
    e = empty_last_split(n)
    if e:
        s.add(e)
    return tuple(sorted(x for x in s if x >= 1))


def edge_positions(S, n, dtype, hd):
    """First and last position of every split's chunk and both sides of every batch boundary inside a chunk, for a row of S."""
    B = batch(dtype, hd)
    edges = set()
    for p0, p1 in splits(S, n):
        if p0 < p1:
            edges |= {p0, p1 - 1}
            for b in range(p0 + B, p1, B):
                edges |= {b - 1, b}
    return edges


def pick(keep, edges, lo, hi, count, rng):
    """`count` positions of [lo, hi): all of `keep`, then of `edges` (sampled down where there are more), then random ones."""
    keep = {int(p) for p in keep if lo <= p < hi}
    edges = sorted({int(p) for p in edges if lo <= p < hi} - keep)
    if hi - lo <= count:
        return set(range(lo, hi))
    room = max(count - len(keep), 0)
    if len(edges) > room:
        edges = [int(e) for e in rng.choice(edges, size=room, replace=False)]
    pos = keep | set(edges)
    while len(pos) < count:
        pos.add(int(rng.randint(lo, hi)))
    return pos


def probe_positions(S, n, dtype, hd, rng):
    """The N_PROBES lifted positions of a row of S without a shared prefix."""
    return np.array(sorted(pick({0, S - 1}, edge_positions(S, n, dtype, hd), 0, S, N_PROBES, rng)))


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=4)
def content(hd, n_pos):
    """The flat numbers: q [NQ][H][hd], K / V [2][H][n_pos][hd] - content 0 is what sequence 0 holds, content 1 what every other
    sequence holds (so a read from the wrong side of the prefix boundary reads other numbers even where it meets no NaN)."""
    rng = np.random.RandomState(7 * hd + n_pos)
    q = bf16_exact(rng.uniform(-1, 1, (NQ, H, hd)))
    K = bf16_exact(rng.uniform(-1, 1, (2, H, n_pos, hd)))
    sc = np.einsum("qhd,chsd->qchs", q.astype(np.float64), K.astype(np.float64)) * kernel_scale(hd)
    K = K * np.float32(2.0 ** np.floor(np.log2(0.25 / np.abs(sc).max())))          # a power of two: still bf16-exact
    V = bf16_exact(rng.uniform(0.5, 1.5, K.shape)) * rng.choice(np.float32([-1, 1]), size=K.shape)
    for a in (q, K, V):
        a.setflags(write=False)
    return q, K, V


@dataclass
class Launch:
    dtype: str
    hd: int
    nsplit: int
    family: str
    share: int
    q: np.ndarray             # fp32 [rows][H * hd]
    Kf: np.ndarray            # fp32 [n_seqs][H][S_max + 1][hd], no NaN: what the sequences would hold if they went on (defect models)
    Vf: np.ndarray
    row_seq: np.ndarray       # int32 [rows]
    row_pos: np.ndarray
    covered: list = field(default_factory=list)          # per row: the positions the defect models are applied at

    @property
    def rows(self):
        return len(self.row_pos)

    @property
    def S_max(self):
        return self.Kf.shape[2] - 1

    @property
    def name(self):
        return f"{self.family}-{self.dtype}-hd{self.hd}-n{self.nsplit}-sh{self.share}"


def _along_q(qh, score, hd):
    """K rows [len(score)][hd] whose score against qh is about `score` each: multiples of qh, rounded to bf16."""
    c = np.asarray(score, dtype=np.float64) / (float(qh.astype(np.float64) @ qh.astype(np.float64)) * kernel_scale(hd))
    return bf16_exact(c[:, None] * qh[None, :].astype(np.float64))


def make_launch(dtype, hd, nsplit, family, lengths, share=0, seed=0):
    """Rows of the context lengths `lengths`, row i in sequence (i + 1) % rows: the LAST row is sequence 0's, and with a shared prefix
    it must hold at least `share` positions."""
    lengths = [int(s) for s in lengths]
    rows = len(lengths)
    assert rows >= 2 and min(lengths) >= 1 and (share == 0 or lengths[-1] >= share)
    S_max = max(max(lengths), share)
    cq, cK, cV = content(hd, S_max + 1)
    rng = np.random.RandomState(1000 * seed + 10 * nsplit + hd + len(family) + share)
    row_seq = np.array([(i + 1) % rows for i in range(rows)], dtype=np.int32)
    row_pos = np.array([s - 1 for s in lengths], dtype=np.int32)
    Kf = np.stack([cK[0 if s == 0 else 1] for s in range(rows)]).copy()
    Vf = np.stack([cV[0 if s == 0 else 1] for s in range(rows)]).copy()
    one_q = family == "probe" and share > 0          # lifted prefix rows in sequence 0 serve every row: they need one q direction
    qi = [0 if one_q else i % NQ for i in range(rows)]
    q = np.stack([cq[j].reshape(H * hd) for j in qi])
    covered = []
    prefix = pick({0, share - 1}, edge_positions(max(lengths), nsplit, dtype, hd), 0, share, PREFIX_PROBES, rng) if share else set()
    for i, S in enumerate(lengths):
        s = int(row_seq[i])
        if family == "flat":
            covered.append(np.arange(S))
            continue
        if family == "probe":
            if share == 0:
                pos = probe_positions(S, nsplit, dtype, hd, rng)
            else:          # the prefix's probes are the launch's (every row reads them): PREFIX_PROBES of them, the rest the row's own
                own = pick({share, S - 1}, edge_positions(S, nsplit, dtype, hd), share, S, N_PROBES - PREFIX_PROBES, rng) if S > share else {S - 1}
                pos = np.array(sorted({p for p in prefix if p < S} | own))
            where = np.append(pos, S)          # ... and what pos + 1 would hold, for the defect model that includes it
            for h in range(H):
                rows_k = _along_q(cq[qi[i]][h], np.full(len(where), LIFT), hd)
                for p, kr in zip(where, rows_k):
                    Kf[0 if p < share else s, h, p] = kr
            covered.append(pos)
            continue
        assert family == "peaked" and share == 0
        run = min(RUN, S)
        r0 = int(rng.randint(S - run + 1))
        target = rng.uniform(PEAK_LOW, PEAK_HIGH, S + 1)
        target[r0:r0 + run] = PEAK
        target[S] = PEAK
        for h in range(H):
            Kf[s, h, : S + 1] = _along_q(cq[qi[i]][h], target, hd)
        covered.append(np.arange(r0, r0 + run))
    return Launch(dtype, hd, nsplit, family, share, q, Kf, Vf, row_seq, row_pos, covered)


def kernel_caches(L):
    """K / V as the kernel gets them: fp32 [n_seqs][H][S_max][hd], NaN above each sequence's pos and, in sequences other than 0, below
    the shared prefix."""
    K, V = L.Kf[:, :, : L.S_max].copy(), L.Vf[:, :, : L.S_max].copy()
    for i in range(L.rows):
        s, pos = int(L.row_seq[i]), int(L.row_pos[i])
        for a in (K, V):
            a[s, :, pos + 1:] = np.nan
            if s != 0:
                a[s, :, : L.share] = np.nan
    return K, V


def row_kv(L, K, V, i):
    """The float64 K / V rows [H][S][hd] row i attends to, out of caches K / V."""
    s, pos = int(L.row_seq[i]), int(L.row_pos[i])
    sh = min(L.share, pos + 1) if s else 0
    Kr = np.concatenate([K[0, :, :sh], K[s, :, sh: pos + 1]], axis=1).astype(np.float64)
    Vr = np.concatenate([V[0, :, :sh], V[s, :, sh: pos + 1]], axis=1).astype(np.float64)
    return Kr, Vr


# ------------------------------------------------------------------------------------------------ reference, bars, merge
def row_eval(qr, Kr, Vr, hd):
    """Softmax(q K scale) V of one row in float64; qr [H][hd], Kr / Vr [H][S][hd]."""
    sc = np.einsum("hd,hsd->hs", qr.astype(np.float64), Kr) * kernel_scale(hd)
    m = sc.max(axis=1, keepdims=True)
    e = np.exp(sc - m)
    D = e.sum(axis=1)
    N = np.einsum("hs,hsd->hd", e, Vr)
    return dict(sc=sc, m=m[:, 0], e=e, D=D, N=N, out=N / D[:, None], wabs=np.einsum("hs,hsd->hd", e, np.abs(Vr)) / D[:, None],
                vmax=np.abs(Vr).max(axis=(1, 2)))


def bars(ev, bf16_out):
    """Per-element bar [H][hd] of a row (module docstring)."""
    b = BAR32 * ev["vmax"][:, None] * np.ones_like(ev["out"])
    return b + BAR16 * ev["wabs"] if bf16_out else b


def reference(L, K=None, V=None):
    """Per row: (out [rows][H * hd] float64, fp32-output bar, bf16-output bar), from the caches the kernel is handed."""
    if K is None:
        K, V = kernel_caches(L)
    out, b32, b16 = [], [], []
    for i in range(L.rows):
        Kr, Vr = row_kv(L, K, V, i)
        ev = row_eval(L.q[i].reshape(H, L.hd), Kr, Vr, L.hd)
        out.append(ev["out"].reshape(-1))
        b32.append(bars(ev, False).reshape(-1))
        b16.append(bars(ev, True).reshape(-1))
    return np.stack(out), np.stack(b32), np.stack(b16)


def restate_fp32(L, K=None, V=None):
    """The same rows as a plain fp32 torch restatement (softmax(q K^T scale) V, one pass): its distance from `reference` is what fp32
    arithmetic alone costs, the yardstick printed next to the kernel's figure."""
    if K is None:
        K, V = kernel_caches(L)
    out = []
    for i in range(L.rows):
        Kr, Vr = row_kv(L, K, V, i)
        qr = torch.from_numpy(L.q[i].reshape(H, 1, L.hd))
        w = torch.softmax(qr @ torch.from_numpy(Kr).float().transpose(1, 2) * np.float32(kernel_scale(L.hd)), dim=-1)
        out.append((w @ torch.from_numpy(Vr).float()).reshape(-1).numpy())
    return np.stack(out).astype(np.float64)


def merge(att_o, att_ml):
    """Split partials to rows, in float64: out = sum_i e^(M_i - M) O_i / sum_i e^(M_i - M) L_i over the partials with L_i > 0 (a partial
    with L_i = 0 contributes nothing, whatever its M_i).  att_o [rows][H][n][hd], att_ml [rows][H][n][2] -> [rows][H * hd]; a row
    without any live partial comes out as NaN."""
    O = np.asarray(att_o, dtype=np.float64)
    M = np.asarray(att_ml, dtype=np.float64)[..., 0]
    Ls = np.asarray(att_ml, dtype=np.float64)[..., 1]
    live = Ls > 0
    top = np.where(live, M, -np.inf).max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where(live, np.exp(np.where(live, M - top, 0.0)), 0.0)
    num = (c[..., None] * np.where(live[..., None], O, 0.0)).sum(axis=2)
    den = (c * np.where(live, Ls, 0.0)).sum(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = num / den[..., None]
    return out.reshape(out.shape[0], -1)


def split_partials(qr, Kr, Vr, hd, cuts):
    """Float64 partials of one row under ANY partition `cuts` = [(p0, p1)]: (att_o [H][n][hd], att_ml [H][n][2]), empty pieces as the
    kernel leaves them, (-inf, 0) and zeros.  For testing `merge`."""
    n = len(cuts)
    O, ML = np.zeros((H, n, hd)), np.zeros((H, n, 2))
    ML[..., 0] = -np.inf
    sc = np.einsum("hd,hsd->hs", qr.astype(np.float64), Kr) * kernel_scale(hd)
    for i, (p0, p1) in enumerate(cuts):
        if p0 >= p1:
            continue
        m = sc[:, p0:p1].max(axis=1)
        e = np.exp(sc[:, p0:p1] - m[:, None])
        O[:, i] = np.einsum("hs,hsd->hd", e, Vr[:, p0:p1])
        ML[:, i, 0], ML[:, i, 1] = m, e.sum(axis=1)
    return O, ML


# ------------------------------------------------------------------------------------------------ defect models
MODELS = ("drop", "twice", "neighbour", "beyond", "own_prefix")


def row_sensitivity(L, K, V, i):
    """{model: (sens32, sens16)}: over the covered positions of row i, the SMALLEST of max_j |defective - reference|_j / bar_j, against the
    fp32-output and the bf16-output bar.  A model that does not apply to the row (one position: nothing to drop or swap; sequence 0 or
    no prefix: no own_prefix) is left out."""
    hd = L.hd
    s, pos = int(L.row_seq[i]), int(L.row_pos[i])
    S = pos + 1
    qr = L.q[i].reshape(H, hd)
    Kr, Vr = row_kv(L, K, V, i)
    ev = row_eval(qr, Kr, Vr, hd)
    b32, b16 = bars(ev, False), bars(ev, True)
    e, D, N, out = ev["e"], ev["D"], ev["N"], ev["out"]
    P = np.asarray(L.covered[i])

    def sens(num, den):          # num [H][n][hd], den [H][n] -> (sens32, sens16)
        d = np.abs(num / den[..., None] - out[:, None, :])
        return float((d / b32[:, None, :]).max(axis=(0, 2)).min()), float((d / b16[:, None, :]).max(axis=(0, 2)).min())

    eP, VP = e[:, P], Vr[:, P]                                   # [H][n], [H][n][hd]
    eV = eP[..., None] * VP
    res = {}
    if S > 1:
        res["drop"] = sens(N[:, None] - eV, D[:, None] - eP)
        nb = np.where(P < pos, P + 1, P - 1)
        res["neighbour"] = sens(N[:, None] - eV + e[:, nb][..., None] * Vr[:, nb], D[:, None] - eP + e[:, nb])
        res["twice"] = sens(N[:, None] + eV, D[:, None] + eP)          # (a row of one position is its V whatever its weight)

    def foreign(Kx, Vx):          # weights and values of rows the reference does not hold, on the reference's scale
        ex = np.exp(np.einsum("hd,hnd->hn", qr.astype(np.float64), Kx.astype(np.float64)) * kernel_scale(hd) - ev["m"][:, None])
        return ex, ex[..., None] * Vx.astype(np.float64)

    sx = 0 if S < L.share else s          # where position pos + 1 would be read from
    ex, exV = foreign(L.Kf[sx, :, S:S + 1], L.Vf[sx, :, S:S + 1])
    res["beyond"] = sens(N[:, None] + exV, D[:, None] + ex)
    below = P[P < min(L.share, S)] if s else P[:0]
    if len(below):
        ex, exV = foreign(L.Kf[s][:, below], L.Vf[s][:, below])
        res["own_prefix"] = sens(N[:, None] - e[:, below][..., None] * Vr[:, below] + exV, D[:, None] - e[:, below] + ex)
    return res


def launch_sensitivity(L):
    """{model: (sens32, sens16)}, the minimum over the launch's rows."""
    K, V = kernel_caches(L)
    res = {}
    for i in range(L.rows):
        for k, (a, b) in row_sensitivity(L, K, V, i).items():
            res[k] = (min(a, res[k][0]), min(b, res[k][1])) if k in res else (a, b)
    return res


# ------------------------------------------------------------------------------------------------ the tables
def edge_launches(dtype, hd, nsplit):
    """{family: Launch} of the edge lengths of one (dtype, head_dim, nsplit): flat for the fp32-output forms, probe and peaked for all."""
    ls = edge_lengths(dtype, hd, nsplit)
    return {f: make_launch(dtype, hd, nsplit, f, ls) for f in ("flat", "probe", "peaked")}


def share_values(dtype, hd):
    return (1, ppw(dtype, hd), batch(dtype, hd) + 3, "pos")


SHARE_NSPLITS = (1, 4, 8)


def share_launch(dtype, hd, nsplit, share, family):
    """Rows around a shared prefix: contexts shorter than the prefix, ending at it, one past it, inside the first batch behind it and a
    refill behind it; the last row is sequence 0's own.  share = "pos": the prefix is everything below the longest row's last position."""
    B = batch(dtype, hd)
    top = nsplit * B + 7
    sh = top - 1 if share == "pos" else int(share)
    ls = sorted({max(1, sh - 1), sh, sh + 1, sh + 2, min(top, sh + ppw(dtype, hd) + 1), min(top, sh + B + 1), top})
    return make_launch(dtype, hd, nsplit, family, ls + [top], share=sh, seed=1)


# ------------------------------------------------------------------------------------------------ every length (the sweep)
def sweep_reference(dtype, hd):
    """Flat family, every S = 1 .. sweep_top: out[c][j][S - 1] = the row of q vector j over positions 0..S-1 of content c (0: sequence
    0's numbers, 1: any other sequence's), [2][NQ][top][H * hd] float64 by prefix sums (flat scores need no running maximum), and the
    fp32-output bar [2][top][H] (per head; the same for every element and q)."""
    top = sweep_top(dtype, hd)
    cq, cK, cV = content(hd, top + 1)
    K, V = cK[:, :, :top].astype(np.float64), cV[:, :, :top].astype(np.float64)
    e = np.exp(np.einsum("qhd,chsd->cqhs", cq.astype(np.float64), K) * kernel_scale(hd))
    D = np.cumsum(e, axis=-1)
    N = np.cumsum(e[..., None] * V[:, None], axis=-2)                 # [c][q][H][S][hd]
    out = (N / D[..., None]).transpose(0, 1, 3, 2, 4).reshape(2, NQ, top, H * hd)
    bar = BAR32 * np.maximum.accumulate(np.abs(V).max(axis=-1), axis=-1).transpose(0, 2, 1)      # [c][S][H]
    return out, bar


def sweep_launch(dtype, hd, lengths):
    """The sweep's rows of the given lengths as a Launch (flat, no prefix), over the sweep's own content: for the CPU checks."""
    top = sweep_top(dtype, hd)
    cq, cK, cV = content(hd, top + 1)
    rows = len(lengths)
    row_seq = np.array([(i + 1) % rows for i in range(rows)], dtype=np.int32)
    Kf = np.stack([cK[0 if s == 0 else 1] for s in range(rows)])
    Vf = np.stack([cV[0 if s == 0 else 1] for s in range(rows)])
    q = np.stack([cq[(S - 1) % NQ].reshape(-1) for S in lengths])
    return Launch(dtype, hd, 1, "flat", 0, q, Kf, Vf, row_seq, np.array([S - 1 for S in lengths], dtype=np.int32),
                  [np.arange(S) for S in lengths])
