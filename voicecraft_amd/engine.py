"""Python mirror of the reference's model interface for the decode path.

`VoiceCraftEngine` exposes `inference_tts`, `inference_tts_batch` and `inference` with the
signatures, argument meaning, return shapes and AssertionErrors of `models.voicecraft.VoiceCraft`
(models/voicecraft.py:908, :1156, :561), so `inference_tts_scale.inference_one_sample`
(inference_tts_scale.py:42-105) and its editing twin run unchanged on it.  All compute happens in
libvcengine.so (HIP, gfx950) behind the C ABI of include/vc_engine.h; torch is used only to hold
device memory for inputs/outputs, to read the state_dict and to name the current stream.
There is no CPU or eager fallback: without the library every constructor raises.
"""
from __future__ import annotations

import ast
import ctypes as C
import logging
import math
import random
from argparse import Namespace
from collections import namedtuple
from typing import Iterable

import torch

from . import _lib
from ._lib import EngineError, ModelCfg, SampleCfg, check

_DTYPES = {"bf16": _lib.VC_DTYPE_BF16, "bfloat16": _lib.VC_DTYPE_BF16, torch.bfloat16: _lib.VC_DTYPE_BF16,
           "fp32": _lib.VC_DTYPE_F32, "float32": _lib.VC_DTYPE_F32, torch.float32: _lib.VC_DTYPE_F32}


def _sine_table(n: int, d: int) -> torch.Tensor:
    # same torch ops as SinePositionalEmbedding.extend_pe (models/modules/embedding.py:77-90)
    pos = torch.arange(0, n, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(n, d)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe.contiguous()


class VoiceCraftEngine:
    """Drop-in for `VoiceCraft(args)` + `load_state_dict` + `.to(device).eval()` on the inference path.

    Capacities (the reference grows its tensors as it goes; the engine preallocates):
      max_seqs       concurrent sequences (best-of-N samples / utterances of inference_tts_multi)
      max_positions  cached positions per sequence = Lx + prompt columns + generated steps.  A call whose
                     PROMPT does not fit raises EngineError(VC_ECAP) at once; a call whose worst case (the
                     reference's length cap, 10 frames per phoneme) does not fit still runs and raises only
                     if generation really reaches the end of the cache before the terminator.  The default
                     covers Lx <= 370 phonemes in the worst case (11*Lx + 6 positions).
    """

    def __init__(self, args: Namespace | dict, state_dict: dict[str, torch.Tensor], device="cuda:0",
                 dtype="bf16", max_seqs: int = 8, max_positions: int = 4096, use_graph: bool = True, w8: str | None = None,
                 kv8: bool | str = False, w8_rows: bool = False, w8_wide: bool = False,
                 w8_mid: bool = False, w8_up: bool = False, w8_up_rows: bool = False, w8_qkv_rows: bool = False):
        """kv8: False (default: nothing changes) | True | "centred" - decode passes of a bf16 engine read the cached K / V positions older than the pass
        as one E4M3 byte per value times a per-row shift (option `kv8`, csrc/vc_kv8.h, quant.kv8_quantize_rows): half the bytes of the
        launch that grows with the batch, 3 mantissa bits left of a cached value, 1.5 x the K/V memory.  Works with every call and `w8=`.
        "centred" (vc_request_kv8c; quant.kv8c_* state the contract): the same, with K stored as k - c, c the mean K row of the slot's
        prompt per layer and head, and q . c added back to the 8-bit scores - softmax does not see the K rows' common offset, which is
        where the plain grid loses its bits on peaked attention.  Option `kv8` = 0 / 1 switches either mode off and on.
        w8: None (default: nothing changes) | "quantize" | "as_is" - one-row steps of a bf16 engine stream the matrices of W8_MATRICES
        as one E4M3 byte per value (option `w8`, csrc/vc_w8.h), bit-identical to the bf16 launches on the same weights.  "quantize" first
        puts those matrices on the 8-bit grid (quant.quantize_state_dict_w8, on the CPU) and keeps the result as `self.w8_state_dict`,
        the checkpoint this engine then computes; "as_is" takes the weights as given: a matrix off the grid comes back refused
        (w8_stats()) and keeps its bf16 launch.
        w8_rows: False (default: nothing changes) | True, with `w8=` only (ValueError without it) - steps of 2..8 rows stream the same
        bytes too (option `w8r`, mask W8_ROWS_MASK: the FFN down-projection at d = 512 / 1024 / 2048, the QKV projection of layers 1..
        at d = 2048 up to 6 rows), bit-identical to the image launches; launch_counts()["w8_rows"] counts them.
        w8_wide: False (default: nothing changes) | True, with `w8=` only (ValueError without it) - on an engine that runs wide steps
        (max_seqs > 16) the FFN down-projection and the QKV projection of 17..64-row steps stream E4M3 bytes too (option `w8w`, mask
        W8_WIDE_MASK; pair planes of the 16-channel images, csrc/vc_w8.h: + 0.5 x the two images resident, + 0.47 GB at giga830M),
        bit-identical to the image launches; launch_counts()["w8_wide"] counts them, w8_stats() says which layers have the planes.
        w8_mid: False (default: nothing changes) | True, with `w8=` only (ValueError without it) - passes of 9..16 rows stream the FFN
        down-projection from the same bytes as the one-row step (option `w8m`, mask W8_MID_MASK; d = 512 / 1024 / 2048; nothing more is
        packed, resident memory does not change), bit-identical to the image launches; launch_counts()["w8_mid"] counts them.
        w8_up: False (default: nothing changes) | True, with `w8=` only (ValueError without it) - on an engine that runs wide steps
        (max_seqs > 16) the FFN up-projection of 17..64-row steps streams E4M3 bytes (option `w8u`, mask W8_UP_MASK; pair planes of the
        16-channel image of linear1.weight folded with norm2.weight: + 0.5 x that image resident, + 0.27 GB at giga830M; d = 512 / 1024
        / 2048), bit-identical to the image launch on the same weights; launch_counts()["w8_up"] counts them, w8_stats() says which
        layers have the planes.  This is a third matrix on the 8-bit grid: `w8="quantize"` then quantises it too (`w8_state_dict` is
        that checkpoint, which steps of every width compute: narrower steps read its bf16 image), `w8="as_is"` takes the weights as
        given and a layer off the grid keeps its image launch.  Independent of w8_wide, w8_rows, w8_mid and kv8.
        w8_up_rows: False (default: nothing changes) | True, with `w8=` only (ValueError without it) - the FFN up-projection of passes of
        2..16 rows streams the same E4M3 pair planes (option `w8ur`, mask W8_UP_ROWS_MASK; d = 512 / 1024 / 2048), packed whatever
        max_seqs is: + 0.27 GB at giga830M on an engine that does not hold them for `w8_up` already, nothing next to it.  Bit-identical
        to the image launch on the same weights; launch_counts()["w8_up_rows"] counts them, w8_stats() says which layers have the
        planes.  `w8="quantize"` quantises the third matrix as for w8_up.  Independent of w8_up, w8_wide, w8_rows, w8_mid and kv8.
        w8_qkv_rows: False (default: nothing changes) | True, with `w8=` only (ValueError without it) - the QKV projection of the
        finished-row passes that still read the 12-channel bf16 image (9..16 rows; 7 and 8 at d = 2048) streams E4M3 pairs of that image
        for layers 1.. (option `w8q`, mask W8_QKV_ROWS_MASK; d = 512 / 1024 / 2048), packed whatever max_seqs is: + 0.20 GB at giga830M.
        Bit-identical to the image launch on the same weights; launch_counts()["w8_qkv_rows"] counts them, w8_stats() says which
        layers have the pairs.  No new matrix is quantised (QKV is one of W8_MATRICES).  Independent of the other w8 keywords and kv8."""
        self.lib = _lib.load()
        asked = dict(w8_rows=w8_rows, w8_mid=w8_mid, w8_wide=w8_wide, w8_up=w8_up, w8_up_rows=w8_up_rows, w8_qkv_rows=w8_qkv_rows)
        for form in reversed(self.W8_FORMS):      # (the newest keyword is named first, as it always was)
            if asked[form.keyword] and w8 is None:
                raise ValueError(f'{form.keyword}=True streams planes on the grid of `w8=`: give w8="quantize" or w8="as_is" too')
        if isinstance(kv8, str) and kv8 != "centred":
            raise ValueError(f'kv8 = {kv8!r}: False, True or "centred"')
        a = Namespace(**args) if isinstance(args, dict) else Namespace(**vars(args))
        # the same normalisation VoiceCraft.__init__ applies (models/voicecraft.py:117-127)
        if not getattr(a, "special_first", False):
            a.special_first = 0
        if not getattr(a, "n_special", False):
            a.n_special = 3
        a.eos = getattr(a, "eos", -1)
        if isinstance(a.audio_vocab_size, str):
            a.audio_vocab_size = int(ast.literal_eval(a.audio_vocab_size))   # the reference eval()s it (voicecraft.py:126-127)
        assert a.text_pad_token == a.text_vocab_size, (a.text_vocab_size, a.text_pad_token)
        assert a.audio_vocab_size == a.empty_token, a.empty_token
        assert a.eog == a.audio_vocab_size + 1, a.eog
        assert a.audio_pad_token == a.audio_vocab_size + 2, a.audio_pad_token
        if a.eos > 0:
            assert a.eos != a.audio_pad_token and a.eos != a.empty_token, a.eos
        # vc_create refuses one codebook too: the reference's TTS cuts the shifted prompt with [:, :-(n_codebooks-1)]
        # (models/voicecraft.py:967, :1217), which at K = 1 is [:, :-0] - the whole audio prompt is dropped, so there is no result to equal
        assert int(a.n_codebooks) >= 2, (f"n_codebooks {a.n_codebooks} unsupported: the reference's own TTS drops the whole audio prompt "
                                         "at one codebook ([:, :-(n_codebooks-1)]); 2..8 are supported")
        self.args = a
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("VoiceCraftEngine runs on an MI355X only (device must be cuda:N); there is no CPU path")
        self.compute_dtype = _DTYPES[dtype]
        self.use_graph = bool(use_graph)
        self.max_seqs, self.max_positions = int(max_seqs), int(max_positions)
        cfg = ModelCfg(
            d_model=a.d_model, nhead=a.nhead, num_layers=a.num_decoder_layers, n_codebooks=a.n_codebooks,
            audio_vocab_size=a.audio_vocab_size, n_special=int(a.n_special), text_rows=a.text_vocab_size + 1,
            head_hidden=a.audio_vocab_size // 2, empty_token=a.empty_token, eog=a.eog,
            audio_pad_token=a.audio_pad_token, eos=a.eos if a.eos > 0 else -1,
            reduced_eog=int(getattr(a, "reduced_eog", 0) or 0), encodec_sr=int(a.encodec_sr),
            max_n_spans=int(a.max_n_spans), max_seqs=self.max_seqs, max_positions=self.max_positions)
        self._h = C.c_void_p()
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        assert w8 in (None, "quantize", "as_is"), f'w8 = {w8!r}: None, "quantize" or "as_is"'
        self.w8_state_dict = None
        if w8 == "quantize":
            from . import quant
            state_dict = self.w8_state_dict = quant.quantize_state_dict_w8(a, state_dict, self.W8_MATRICES, ffn_up=bool(w8_up or w8_up_rows))
        check(self.lib.vc_create(C.byref(cfg), index, C.byref(self._h)), None, "vc_create")
        if w8 is not None:
            check(self.lib.vc_request_w8(self._h, self.W8_MASK), self._h, "vc_request_w8")
        for form in self.W8_FORMS:                # self.w8_rows .. self.w8_qkv_rows: what w8_stats() reports
            setattr(self, form.keyword, bool(asked[form.keyword]))
            if asked[form.keyword]:
                check(getattr(self.lib, form.request)(self._h, getattr(self, form.mask)), self._h, form.request)
        self.kv8 = bool(kv8)
        self.kv8_centred = kv8 == "centred"
        if self.kv8_centred:
            check(self.lib.vc_request_kv8c(self._h), self._h, "vc_request_kv8c")
        elif self.kv8:
            check(self.lib.vc_request_kv8(self._h), self._h, "vc_request_kv8")
        self._load(state_dict)
        self.last_steps = 0
        self.last_kept: list[int] = []       # inference_tts_multi / _long with batch_size > 1: kept sample per utterance

    # ------------------------------------------------------------------ nn.Module look-alikes
    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self.lib.vc_destroy(h)
            except Exception:  # pragma: no cover
                pass

    # ------------------------------------------------------------------ weights
    def _load(self, state_dict) -> None:
        keep = []
        for key, t in state_dict.items():
            if not torch.is_tensor(t) or not t.is_floating_point():
                continue                      # eog / eos buffers, torchmetrics state
            if key.startswith("accuracy_metrics"):
                continue
            t = t.detach().to(torch.float32).contiguous()
            keep.append(t)
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
            check(self.lib.vc_load_tensor(self._h, key.encode(), C.c_void_p(t.data_ptr()), int(t.is_cuda),
                                          _lib.VC_DTYPE_F32, shape, t.dim()), self._h, f"vc_load_tensor({key})")
        pe = _sine_table(self.max_positions, self.args.d_model)
        shape = (C.c_int64 * 2)(*pe.shape)
        check(self.lib.vc_load_tensor(self._h, b"pe", C.c_void_p(pe.data_ptr()), 0, _lib.VC_DTYPE_F32, shape, 2),
              self._h, "vc_load_tensor(pe)")
        check(self.lib.vc_finalize_weights(self._h, self.compute_dtype), self._h, "vc_finalize_weights")

    # ------------------------------------------------------------------ helpers
    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _sample_cfg(self, top_k, top_p, temperature, stop_repetition, silence_tokens, seed=None,
                    forced_mode="tokens") -> SampleCfg:
        sc = SampleCfg()
        sc.forced_mode = {"tokens": 0, "draws": 1}[forced_mode]
        sc.top_k = int(top_k)
        sc.top_p = float(top_p)
        sc.temperature = float(temperature)
        sc.stop_repetition = int(stop_repetition)
        sil = list(silence_tokens)
        assert len(sil) <= _lib.VC_MAX_SILENCE, f"at most {_lib.VC_MAX_SILENCE} silence tokens are supported, got {len(sil)}"
        sc.n_silence = len(sil)
        for i, v in enumerate(sil):
            sc.silence_tokens[i] = int(v)
        # the reference draws from torch's global generator (seed_everything, inference_tts_scale.py:128-135);
        # one draw from it keys the device Philox stream, so torch.manual_seed still makes runs repeatable
        sc.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        sc.use_graph = int(self.use_graph)
        sc.poll_every = 0
        return sc

    def _prep(self, x, x_lens, y):
        assert x.ndim == 2, x.shape
        assert x_lens.ndim == 1, x_lens.shape
        assert y.ndim == 3, y.shape
        if self.args.special_first:
            y = y + int(self.args.n_special)
        assert y.shape[0] == 1 and y.shape[2] == self.args.n_codebooks, y.shape
        assert x.shape[0] == 1, x.shape
        Lx = int(x_lens[0])
        xd = x[0, :Lx].to(self.device, torch.int64).contiguous()
        yd = y[0].to(self.device, torch.int64).contiguous()          # [T,K], time-major as given
        return xd, Lx, yd, int(yd.shape[0])

    def _forced_arg(self, forced, B: int):
        """[steps,K] or [steps,B,K] int64 -> (device tensor kept alive by the caller, pointer, n_steps)."""
        if forced is None:
            return None, None, 0
        K = self.args.n_codebooks
        fd = torch.as_tensor(forced, dtype=torch.int64).reshape(-1, B, K).to(self.device).contiguous()
        return fd, C.c_void_p(fd.data_ptr()), int(fd.shape[0])

    def _gen_budget(self, Lx: int, n_cols: int, mult: int, spans: int = 1) -> int:
        K = self.args.n_codebooks
        return max(0, Lx * mult - n_cols + 1) + spans * (K + 4) + 8

    # ------------------------------------------------------------------ TTS
    @torch.no_grad()
    def inference_tts(self, x, x_lens, y, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0,
                      stop_repetition: int = 3, kvcache: int = 1, silence_tokens: Iterable[int] = (1388, 1898, 131),
                      *kargs, _n_samples: int = 1, _forced=None, _logit_steps: int = 0, _seed=None,
                      _forced_mode: str = "tokens"):
        """models/voicecraft.py:908.  `kvcache` is accepted and ignored: the cache is always on
        (kvcache=0 and kvcache=1 give identical tokens in the reference)."""
        xd, Lx, yd, T = self._prep(x, x_lens, y)
        logging.info(f"silence tokens: {list(silence_tokens)}, note that if you are not using the pretrained encodec 6f79c6a8, make sure you specified it yourself, rather than using the default")
        K = self.args.n_codebooks
        sc = self._sample_cfg(top_k, top_p, temperature, stop_repetition, silence_tokens, _seed, _forced_mode)
        cap = T + self._gen_budget(Lx, T + 1, self.args.encodec_sr // 5)
        res = torch.empty((K, cap), dtype=torch.int64, device=self.device)
        nb = int(_n_samples)
        fd, forced_ptr, n_forced = self._forced_arg(_forced, nb)
        logits = None
        if _logit_steps > 0:
            V = self.args.audio_vocab_size + int(self.args.n_special)
            logits = torch.zeros((_logit_steps, nb, K, V), dtype=torch.float32, device=self.device)
        gen_len, n_steps = C.c_int(0), C.c_int(0)
        rc = self.lib.vc_tts(self._h, C.c_void_p(xd.data_ptr()), Lx, C.c_void_p(yd.data_ptr()), T, C.byref(sc),
                             int(_n_samples), forced_ptr, n_forced, C.c_void_p(res.data_ptr()), cap, C.byref(gen_len),
                             C.c_void_p(logits.data_ptr()) if logits is not None else None, int(_logit_steps),
                             C.byref(n_steps), self._stream())
        check(rc, self._h, "vc_tts")
        self.last_steps = n_steps.value
        Tg = gen_len.value
        out = res[:, : T + Tg].unsqueeze(0)
        gen = res[:, T: T + Tg].unsqueeze(0)
        expected_y_len = T + Tg
        assert out.shape == torch.Size((1, K, expected_y_len)), out.shape
        if self.args.special_first:
            out, gen = out - int(self.args.n_special), gen - int(self.args.n_special)
        if logits is not None:
            return out, gen, (logits[:, 0] if nb == 1 else logits)
        return out, gen

    def inference_tts_stream(self, x, x_lens, y, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0,
                             stop_repetition: int = 3, kvcache: int = 1, silence_tokens: Iterable[int] = (1388, 1898, 131),
                             *kargs, chunk_frames: int = 8, _n_samples: int = 1, _seed=None, _forced=None,
                             _forced_mode: str = "tokens"):
        """inference_tts as a generator: yields (first_frame, codes [1, K, n]) while the decode loop runs, every chunk of at
        least `chunk_frames` frames except the last; the chunks are contiguous from frame 0 and their concatenation is `gen` of
        inference_tts with the same arguments.  After exhaustion `self.last_stream_result` holds the (res, gen) pair
        inference_tts would have returned.  Closing the generator early aborts the call and leaves the engine usable.  One
        utterance, one sample: best-of-N (inference_tts_batch) cannot stream - the kept sample is unknown until it terminates."""
        if int(_n_samples) != 1:
            raise AssertionError("inference_tts_stream: best-of-N (n_samples > 1, inference_tts_batch) cannot be streamed: "
                                 "which sample is kept is unknown until one terminates")
        assert int(chunk_frames) >= 1, chunk_frames
        return self._tts_stream(x, x_lens, y, top_k, top_p, temperature, stop_repetition, silence_tokens, int(chunk_frames),
                                _seed, _forced, _forced_mode)

    @torch.no_grad()
    def _tts_stream(self, x, x_lens, y, top_k, top_p, temperature, stop_repetition, silence_tokens, chunk, seed, forced, forced_mode):
        xd, Lx, yd, T = self._prep(x, x_lens, y)
        K = self.args.n_codebooks
        sc = self._sample_cfg(top_k, top_p, temperature, stop_repetition, silence_tokens, seed, forced_mode)
        budget = self._gen_budget(Lx, T + 1, self.args.encodec_sr // 5)
        cap = T + budget
        fd, forced_ptr, n_forced = self._forced_arg(forced, 1)
        shift = int(self.args.n_special) if self.args.special_first else 0
        self.last_stream_result = None
        rc = self.lib.vc_tts_stream_begin(self._h, C.c_void_p(xd.data_ptr()), Lx, C.c_void_p(yd.data_ptr()), T, C.byref(sc),
                                          forced_ptr, n_forced, self._stream())
        check(rc, self._h, "vc_tts_stream_begin")
        finished = False
        side = torch.cuda.Stream(device=self.device) if shift else None
        try:
            ccap = max(chunk, budget + K)
            first, n, done = C.c_int(0), C.c_int(0), C.c_int(0)
            while not done.value:
                buf = torch.empty((K, ccap), dtype=torch.int64, device=self.device)
                check(self.lib.vc_tts_stream_next(self._h, chunk, C.c_void_p(buf.data_ptr()), ccap, C.byref(first), C.byref(n),
                                                  C.byref(done)), self._h, "vc_tts_stream_next")
                if n.value or not done.value:
                    codes = buf[:, : n.value]
                    if shift:
                        # not on the null stream: a launch there would wait for the decode batches queued on the engine's stream
                        with torch.cuda.stream(side):
                            codes = codes - shift
                        side.synchronize()
                    yield first.value, codes.unsqueeze(0)     # final on the device: usable from any stream
            res = torch.empty((K, cap), dtype=torch.int64, device=self.device)
            gen_len, n_steps = C.c_int(0), C.c_int(0)
            finished = True
            check(self.lib.vc_tts_stream_end(self._h, C.c_void_p(res.data_ptr()), cap, C.byref(gen_len), C.byref(n_steps)),
                  self._h, "vc_tts_stream_end")
            self.last_steps = n_steps.value
            Tg = gen_len.value
            self.last_stream_result = (res[:, : T + Tg].unsqueeze(0) - shift, res[:, T: T + Tg].unsqueeze(0) - shift)
        finally:
            if not finished:      # closed early (or an error): abort, the engine stays usable
                self.lib.vc_tts_stream_end(self._h, None, 0, None, None)
            del fd, xd, yd

    @torch.no_grad()
    def inference_tts_batch(self, x, x_lens, y, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0,
                            stop_repetition: int = 3, kvcache: int = 1, batch_size: int = 5,
                            silence_tokens: Iterable[int] = (1388, 1898, 131), *kargs, _seed=None, _forced=None,
                            _forced_mode: str = "tokens", _logit_steps: int = 0):
        """models/voicecraft.py:1156 — best-of-N sampling of ONE utterance; returns the kept sample."""
        return self.inference_tts(x, x_lens, y, top_k, top_p, temperature, stop_repetition, kvcache,
                                  silence_tokens, _n_samples=int(batch_size), _seed=_seed, _forced=_forced,
                                  _forced_mode=_forced_mode, _logit_steps=_logit_steps)

    @torch.no_grad()
    def inference_tts_multi(self, xs, ys, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0,
                            stop_repetition: int = 3, silence_tokens: Iterable[int] = (1388, 1898, 131), _seed=None,
                            _forced=None, _forced_mode: str = "tokens", _logit_steps: int = 0, _shared_text_prefix: int = 0,
                            batch_size: int = 1):
        """B different utterances as one batch (not in the reference: SURVEY.md §8f-1).
        xs: list of int64 [Lx_i]; ys: list of int64 [T_i,K].  Returns list of (res [1,K,T_i+Tg_i], gen)
        (+ the raw head logits [steps,B*N,K,V] as a second value when _logit_steps > 0).
        batch_size N > 1: best-of-N per utterance, as inference_tts_batch(batch_size=N) on each prompt
        (include/vc_engine.h vc_tts_multi_best_of): B*N sequences, sample j of utterance u in slot u*N + j; the kept
        sample's (res, gen) is returned and self.last_kept lists the kept sample index of every utterance.
        _forced is [steps][B*N][K], utterance-major."""
        B = len(xs)
        N = int(batch_size)
        assert N >= 1, f"batch_size must be at least 1, got {batch_size}"
        assert B == len(ys) and 1 <= B <= self.max_seqs, (B, self.max_seqs)
        K = self.args.n_codebooks
        xcat = torch.cat([torch.as_tensor(v, dtype=torch.int64).reshape(-1) for v in xs]).to(self.device).contiguous()
        ycat = torch.cat([torch.as_tensor(v, dtype=torch.int64).reshape(-1, K) for v in ys]).to(self.device).contiguous()
        if self.args.special_first:
            ycat = ycat + int(self.args.n_special)
        xo, yo = [0], [0]
        cap = 0
        for xv, yv in zip(xs, ys):
            Lx, T = int(torch.as_tensor(xv).numel()), int(torch.as_tensor(yv).reshape(-1, K).shape[0])
            xo.append(xo[-1] + Lx)
            yo.append(yo[-1] + T)
            cap = max(cap, T + self._gen_budget(Lx, T + 1, self.args.encodec_sr // 5))
        x_off = (C.c_int32 * (B + 1))(*xo)
        y_off = (C.c_int32 * (B + 1))(*yo)
        sc = self._sample_cfg(top_k, top_p, temperature, stop_repetition, silence_tokens, _seed, _forced_mode)
        res = torch.empty((B, K, cap), dtype=torch.int64, device=self.device)
        gen_len = (C.c_int * B)()
        kept = (C.c_int * B)()
        n_steps = C.c_int(0)
        fd, forced_ptr, n_forced = self._forced_arg(_forced, B * N)
        logits = None
        if _logit_steps > 0:
            V = self.args.audio_vocab_size + int(self.args.n_special)
            logits = torch.zeros((_logit_steps, B * N, K, V), dtype=torch.float32, device=self.device)
        rc = self.lib.vc_tts_multi_best_of(self._h, B, N, C.c_void_p(xcat.data_ptr()), x_off, C.c_void_p(ycat.data_ptr()), y_off,
                                           C.byref(sc), int(_shared_text_prefix), forced_ptr, n_forced, C.c_void_p(res.data_ptr()),
                                           cap, gen_len, kept, C.c_void_p(logits.data_ptr()) if logits is not None else None,
                                           int(_logit_steps), C.byref(n_steps), self._stream())
        check(rc, self._h, "vc_tts_multi")
        self.last_steps = n_steps.value
        self.last_kept = [int(kept[b]) for b in range(B)]
        outs = []
        for b in range(B):
            T, Tg = yo[b + 1] - yo[b], gen_len[b]
            r, g = res[b, :, : T + Tg].unsqueeze(0), res[b, :, T: T + Tg].unsqueeze(0)
            if self.args.special_first:
                r, g = r - int(self.args.n_special), g - int(self.args.n_special)
            outs.append((r, g))
        if logits is not None:
            return outs, logits
        return outs

    # ---- decode sessions: continuous batching (include/vc_engine.h vc_session_*)
    def open_session(self, max_live: int | None = None, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0,
                     stop_repetition: int = 3, silence_tokens: Iterable[int] = (1388, 1898, 131), max_samples: int = 1,
                     **unsupported) -> "DecodeSession":
        """A decode session over `max_live` K/V slots (default max_seqs): TTS requests with inference_tts semantics and editing
        requests with inference semantics, submitted at any time, each joining the running batch between two graph batches and
        handed back as soon as it ends.  max_samples > 1 opens it for best-of-N TTS requests as well (DecodeSession.submit(...,
        n_samples=N), N <= max_samples <= max_live: inference_tts_batch(batch_size=N) semantics, one ticket, N slots); its steps
        then end in two sampler launches instead of one.  top_k / top_p / temperature / stop_repetition given here are the default of a
        request that brings none of its own (DecodeSession.submit / submit_edit); silence_tokens are the session's; the seed is per
        request.  Use it as a context manager.
        A shared text prefix, logits_out and forced trajectories are not part of a session and are refused."""
        if unsupported:
            raise AssertionError(f"open_session: {sorted(unsupported)} not supported - a decode session takes TTS and editing requests "
                                 "(best-of-N is per request: open_session(max_samples=N), submit(n_samples=N), not batch_size; no "
                                 "_shared_text_prefix, no _logit_steps, no _forced trajectories): use the blocking calls for those")
        max_live = self.max_seqs if max_live is None else int(max_live)
        assert 1 <= int(max_samples) <= max_live, f"open_session: max_samples {max_samples} outside [1, max_live = {max_live}]"
        return DecodeSession(self, max_live, self._sample_cfg(top_k, top_p, temperature, stop_repetition, silence_tokens, 0),
                             max_samples=int(max_samples))

    @torch.no_grad()
    def inference_tts_queue(self, xs, ys, max_live: int | None = None, seeds=None, batch_size: int = 1, **sampling):
        """Any number of utterances through `max_live` slots of one decode session (default max_seqs): a freed slot is refilled with
        the next utterance while the others go on decoding.  xs: list of int64 [Lx_i]; ys: list of int64 [T_i,K]; seeds: one per
        utterance (default: drawn from torch's generator, as _sample_cfg does).  Returns the list of (res [1,K,T_i+Tg_i], gen) in
        input order - the return type of inference_tts_multi.  self.last_session_stats holds the session's stats().
        batch_size N > 1: best-of-N per utterance, as inference_tts_multi(batch_size=N) - every utterance is a request of N samples
        (N slots), the kept samples' (res, gen) are returned and self.last_kept lists the kept sample index of every utterance."""
        assert len(xs) == len(ys) and len(xs) >= 1, (len(xs), len(ys))
        assert seeds is None or len(seeds) == len(xs), "one seed per utterance"
        N = int(batch_size)
        assert N >= 1, f"batch_size must be at least 1, got {batch_size}"
        K = self.args.n_codebooks
        with self.open_session(max_live, max_samples=N, **sampling) as sess:
            tickets = []
            for i, (xv, yv) in enumerate(zip(xs, ys)):
                xv = torch.as_tensor(xv, dtype=torch.int64).reshape(1, -1)
                yv = torch.as_tensor(yv, dtype=torch.int64).reshape(1, -1, K)
                tickets.append(sess.submit(xv, torch.tensor([xv.shape[1]]), yv, seed=None if seeds is None else seeds[i], n_samples=N))
            done = {t: (res, gen) for t, res, gen in sess.drain()}
            self.last_session_stats = sess.stats()
            if N > 1:
                self.last_kept = [sess.kept[t] for t in tickets]
        return [done[t] for t in tickets]

    @torch.no_grad()
    def inference_queue(self, xs, ys, mask_intervals, max_live: int | None = None, seeds=None, **sampling):
        """Any number of editing requests through `max_live` slots of one decode session (default max_seqs), each following
        `inference` exactly.  xs, ys, mask_intervals as inference_multi takes them; seeds: one per request.  Sampling defaults are
        `inference`'s (stop_repetition -1).  Returns the list of res [1,K,T'_i] in input order - the return type of
        inference_multi.  self.last_session_stats holds the session's stats()."""
        assert len(xs) == len(ys) == len(mask_intervals) and len(xs) >= 1, (len(xs), len(ys), len(mask_intervals))
        assert seeds is None or len(seeds) == len(xs), "one seed per request"
        K = self.args.n_codebooks
        sampling.setdefault("stop_repetition", -1)
        with self.open_session(max_live, **sampling) as sess:
            tickets = []
            for i, (xv, yv, mi) in enumerate(zip(xs, ys, mask_intervals)):
                xv = torch.as_tensor(xv, dtype=torch.int64).reshape(1, -1)
                yv = torch.as_tensor(yv, dtype=torch.int64).reshape(1, -1, K)
                mi = torch.as_tensor(mi, dtype=torch.int64)
                mi = mi.reshape(1, -1, 2) if mi.ndim == 2 else mi
                tickets.append(sess.submit_edit(xv, torch.tensor([xv.shape[1]]), yv, mi, seed=None if seeds is None else seeds[i],
                                                _who=f"request {i}: "))
            done = {t: res for t, res, gen in sess.drain()}
            self.last_session_stats = sess.stats()
        return [done[t] for t in tickets]

    # ---- the training objective, teacher-forced
    @torch.no_grad()
    def forward(self, batch, mask_intervals=None, mask_values=None, _per_row: bool = False, mask_sampler=None):
        """`VoiceCraft.forward` (models/voicecraft.py:472-559) as an evaluation pass: batch = {"x" [B,Lx], "x_lens" [B],
        "y" [B,K,T], "y_lens" [B]} exactly as the reference's collate gives it; returns the reference's dict
        (`loss` = sum over codebooks of weight * summed cross-entropy, `top10acc`, `top10acc_by_codebook`,
        `effective_ntoken`).  The reference SAMPLES the masked spans inside (`prepare_mask_intervals`, :198-237 - training
        data augmentation, out of this engine's scope); here they are an argument: `mask_intervals[i]` = the (start, end)
        frame pairs of utterance i.  `mask_values[i]` = the utterance's `emb_inds_use` (default 0..M-1; the reference
        shuffles them when `shuffle_mask_embedding` is set).  `mask_sampler`: a callable `y_lens -> mask_intervals` used when
        `mask_intervals` is None (the reference's own `prepare_mask_intervals` fits).  No gradients: this engine does not train.
        `_per_row` (parity hook): also returns, in the engine's row order (utterances back to back, each padded to 16 rows, text rows
        first), `_nll_rows` / `_tgt_rows` [rows, K] and `_logit_rows` [rows, K, V], the head logits of every row (host, fp32)."""
        import ast
        import random
        if mask_intervals is None and mask_sampler is not None:
            # `model(batch)` of the reference draws the spans itself (prepare_mask_intervals, models/voicecraft.py:198-237: random
            # training-time augmentation).  The sampler is not part of this engine, but evaluation code that owns one can hand it in:
            # mask_sampler(y_lens) -> one list of (start, end) frame pairs per utterance, e.g. the bound method
            # `reference_model.prepare_mask_intervals` (same argument, same return value)
            mask_intervals = [[(int(s0), int(e0)) for (s0, e0) in iv] for iv in mask_sampler(batch["y_lens"])]
        if mask_intervals is None:
            raise TypeError("VoiceCraftEngine.forward(batch, mask_intervals=... | mask_sampler=...): the masked spans are an argument here - "
                            "pass one list of (start, end) frame pairs per utterance, or a callable that draws them from y_lens (the "
                            "reference samples them inside prepare_mask_intervals, which this inference engine does not reproduce)")
        x, x_lens, y, y_lens = batch["x"], batch["x_lens"], batch["y"], batch["y_lens"]
        if len(x) == 0:
            return None
        K = self.args.n_codebooks
        assert x.ndim == 2, x.shape
        assert x_lens.ndim == 1, x_lens.shape
        assert y.ndim == 3 and y.shape[1] == K, y.shape
        assert y_lens.ndim == 1, y_lens.shape
        B = int(x.shape[0])
        assert B <= self.max_seqs, (B, self.max_seqs)
        assert mask_intervals is not None and len(mask_intervals) == B, "one list of (start, end) spans per utterance"
        if mask_values is None:
            mask_values = []
            for iv in mask_intervals:
                inds = list(range(self.args.max_n_spans))
                if getattr(self.args, "shuffle_mask_embedding", 0):
                    random.shuffle(inds)                                   # insert_mask, :270-272
                mask_values.append(inds[: len(iv)])
        xs = [x[i, : int(x_lens[i])].to(torch.int64).reshape(-1) for i in range(B)]
        ys = [y[i, :, : int(y_lens[i])].to(torch.int64).transpose(0, 1).reshape(-1, K) for i in range(B)]     # time-major
        xcat = torch.cat(xs).to(self.device).contiguous()
        ycat = torch.cat(ys).to(self.device).contiguous()
        if self.args.special_first:
            ycat = ycat + int(self.args.n_special)
        xo, yo, so = [0], [0], [0]
        flat_iv, flat_mv = [], []
        rows_cap = 0
        for i in range(B):
            xo.append(xo[-1] + int(xs[i].numel()))
            yo.append(yo[-1] + int(ys[i].shape[0]))
            M = len(mask_intervals[i])
            assert M == len(mask_values[i]) and M >= 1, (M, mask_values[i])
            so.append(so[-1] + M)
            for (s0, e0) in mask_intervals[i]:
                flat_iv += [int(s0), int(e0)]
            flat_mv += [int(v) for v in mask_values[i]]
            rows_cap += ((int(xs[i].numel()) + int(ys[i].shape[0]) + (2 * M + 1) * (K + 1) + 2 * M) + 15) // 16 * 16
        c32 = C.c_int32
        nll_sum = (C.c_double * K)()
        hits = (C.c_int64 * K)()
        n_targets = C.c_int64(0)
        n_rows = C.c_int64(0)
        nll = tgt = None
        if _per_row:
            nll = torch.zeros((rows_cap, K), dtype=torch.float32, device=self.device)
            tgt = torch.full((rows_cap, K), -1, dtype=torch.int32, device=self.device)
        rc = self.lib.vc_eval_forward(self._h, B, C.c_void_p(xcat.data_ptr()), (c32 * (B + 1))(*xo),
                                      C.c_void_p(ycat.data_ptr()), (c32 * (B + 1))(*yo),
                                      (c32 * len(flat_iv))(*flat_iv), (c32 * (B + 1))(*so), (c32 * len(flat_mv))(*flat_mv),
                                      nll_sum, hits, C.byref(n_targets),
                                      C.c_void_p(nll.data_ptr()) if nll is not None else None,
                                      C.c_void_p(tgt.data_ptr()) if tgt is not None else None,
                                      rows_cap if _per_row else 0, C.byref(n_rows), self._stream())
        check(rc, self._h, "vc_eval_forward")
        cw = getattr(self.args, "codebook_weight", None)
        cw = [float(w) for w in ast.literal_eval(cw)] if cw else [1.0] * K
        dev = self.device
        by_cb = [torch.tensor(float(hits[k]), device=dev) for k in range(K)]
        out = {
            "loss": torch.tensor(sum(nll_sum[k] * cw[k] for k in range(K)), dtype=torch.float32, device=dev),
            "top10acc": torch.tensor(float(sum(hits[k] for k in range(K))), device=dev),
            "top10acc_by_codebook": by_cb,
            "effective_ntoken": torch.tensor(int(n_targets.value) * K).to(dev),
        }
        if _per_row:
            out["_nll_rows"], out["_tgt_rows"] = nll[: n_rows.value], tgt[: n_rows.value]
            out["_nll_sum"] = [float(nll_sum[k]) for k in range(K)]
            # the head logits of every row, [rows, K, V] fp32 on the host, in the row order of _nll_rows / _tgt_rows
            out["_logit_rows"] = self.debug_read("eval_logits", (int(n_rows.value), K, self.args.audio_vocab_size + int(self.args.n_special)))
        return out

    @torch.no_grad()
    def inference_tts_long(self, x_prompt, x_sentences, y, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0,
                           stop_repetition: int = 3, silence_tokens: Iterable[int] = (1388, 1898, 131), reuse_prefix: bool = True,
                           _seed=None, batch_size: int = 1):
        """Sentence-chained "Long TTS" (gradio_app.py:231-236, :249-313): the reference synthesises every sentence with
        its own `inference_one_sample` call on the text [transcript of the voice prompt ; sentence] and the SAME audio
        prompt.  Here all sentences are decoded together (chunks of max_seqs: the weights are streamed once per step
        for all of them), each row following inference_tts exactly, and with reuse_prefix the K/V of the shared
        transcript prefix are computed once per chunk and read by every sentence (include/vc_engine.h, vc_tts_multi).

        x_prompt int64 [Lp] phonemes of the voice prompt's transcript, x_sentences list of int64 [Ls_i],
        y int64 [1,T,K] (or [T,K]) codes of the voice prompt.  Returns a list of (res [1,K,T+Tg_i], gen [1,K,Tg_i]).
        batch_size = the app's sample_batch_size (gradio_app.py:506, default 3 there): best-of-N per sentence, as its
        inference_one_sample -> inference_tts_batch; sentences then go max_seqs // batch_size per call and
        self.last_kept holds the kept sample index of every sentence."""
        N = int(batch_size)
        assert 1 <= N <= self.max_seqs, f"batch_size {batch_size} must be in [1, max_seqs = {self.max_seqs}]"
        xp = torch.as_tensor(x_prompt, dtype=torch.int64).reshape(-1)
        K = self.args.n_codebooks
        yy = torch.as_tensor(y, dtype=torch.int64).reshape(-1, K)
        outs, kept = [], []
        per_call = self.max_seqs // N
        for c0 in range(0, len(x_sentences), per_call):
            chunk = x_sentences[c0: c0 + per_call]
            xs = [torch.cat([xp, torch.as_tensor(v, dtype=torch.int64).reshape(-1)]) for v in chunk]
            for v in xs:
                assert v.numel() > xp.numel(), "every sentence needs at least one phoneme"
            share = int(xp.numel()) if (reuse_prefix and len(chunk) > 1) else 0
            outs += self.inference_tts_multi(xs, [yy] * len(chunk), top_k, top_p, temperature, stop_repetition, silence_tokens,
                                             _seed=None if _seed is None else _seed + c0, _shared_text_prefix=share, batch_size=N)
            kept += self.last_kept
        self.last_kept = kept
        return outs

    # ------------------------------------------------------------------ editing
    @torch.no_grad()
    def inference(self, x, x_lens, y, mask_interval, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0,
                  stop_repetition: int = -1, kvcache: int = 1, silence_tokens: Iterable[int] = (1388, 1898, 131),
                  _forced=None, _logit_steps: int = 0, _seed=None, _forced_mode: str = "tokens"):
        """models/voicecraft.py:561."""
        xd, Lx, yd, T = self._prep(x, x_lens, y)
        assert mask_interval.shape == torch.Size((1, mask_interval.shape[1], 2)), mask_interval
        logging.info(f"silence tokens: {list(silence_tokens)}, note that if you are not using the pretrained encodec 6f79c6a8, make sure you specified it yourself, rather than using the default")
        K = self.args.n_codebooks
        ivs = [(int(a), int(b)) for a, b in mask_interval[0].tolist()]
        M = len(ivs)
        # insert_mask (models/voicecraft.py:264-288): which mask_embedding row each placeholder uses; a zero-length piece
        # makes the reference raise inside build_pattern_sequence (codebooks_patterns.py:174)
        mask_value = self._edit_layout(ivs, T)
        sc = self._sample_cfg(top_k, top_p, temperature, stop_repetition, silence_tokens, _seed, _forced_mode)
        flat = [v for iv in ivs for v in iv]
        iv_arr = (C.c_int32 * (2 * M))(*flat)
        mv_arr = (C.c_int32 * (2 * M))(*mask_value)
        n_cols = T + 2 * (M + 1) + (M + 1) * K + 1
        cap = T + self._gen_budget(Lx, n_cols, 10, spans=M)
        res = torch.empty((K, cap), dtype=torch.int64, device=self.device)
        fd, forced_ptr, n_forced = self._forced_arg(_forced, 1)
        logits = None
        if _logit_steps > 0:
            V = self.args.audio_vocab_size + int(self.args.n_special)
            logits = torch.zeros((_logit_steps, K, V), dtype=torch.float32, device=self.device)
        res_len, n_steps = C.c_int(0), C.c_int(0)
        rc = self.lib.vc_edit(self._h, C.c_void_p(xd.data_ptr()), Lx, C.c_void_p(yd.data_ptr()), T, iv_arr, M, mv_arr,
                              C.byref(sc), forced_ptr, n_forced, C.c_void_p(res.data_ptr()), cap, C.byref(res_len),
                              C.c_void_p(logits.data_ptr()) if logits is not None else None, int(_logit_steps),
                              C.byref(n_steps), self._stream())
        check(rc, self._h, "vc_edit")
        self.last_steps = n_steps.value
        out = res[:, : res_len.value].unsqueeze(0)
        if self.args.special_first:
            out = out - int(self.args.n_special)
        if logits is not None:
            return out, logits
        return out

    def _edit_layout(self, ivs, T: int, who: str = ""):
        """The per-request part of `inference`: insert_mask's mask_value list (models/voicecraft.py:264-288; one
        `shuffle_mask_embedding` draw per call) and the zero-length-piece IndexError of codebooks_patterns.py:174."""
        M = len(ivs)
        emb_inds = list(range(int(self.args.max_n_spans)))
        if getattr(self.args, "shuffle_mask_embedding", 0):
            random.shuffle(emb_inds)
        use = emb_inds[:M]
        assert len(use) == M, f"{who}{M} spans but max_n_spans is {self.args.max_n_spans}"
        starts = [iv[0] for iv in ivs] + [T]
        ends = [0] + [iv[1] for iv in ivs]
        eos, reduced = self.args.eos, int(getattr(self.args, "reduced_eog", 0) or 0)
        for i, (s, e) in enumerate(zip(ends, starts)):
            has_term = (i == M) if (eos > 0 or reduced) else True
            if e - s + int(has_term) <= 0:
                raise IndexError(f"{who}index is out of bounds for dimension with size 0 (zero-length non-masked piece)")
        return use + use

    @torch.no_grad()
    def inference_multi(self, xs, ys, mask_intervals, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0,
                        stop_repetition: int = -1, silence_tokens: Iterable[int] = (1388, 1898, 131), _seed=None,
                        _forced=None, _forced_mode: str = "tokens", _logit_steps: int = 0):
        """B speech-editing requests as one batch (not in the reference; include/vc_engine.h vc_edit_multi): each follows
        `inference` exactly.  xs: list of int64 [Lx_i]; ys: list of time-major [T_i,K]; mask_intervals: list of per-request
        (start, end) pair lists or [1,M_i,2] tensors.  Returns a list of res [1,K,T'_i] (+ the raw head logits [steps,B,K,V]
        when _logit_steps > 0).  Sampling parameters are shared by the whole call."""
        B = len(xs)
        assert B >= 1 and B == len(ys) == len(mask_intervals), (B, len(ys), len(mask_intervals))
        K = self.args.n_codebooks
        xl = [torch.as_tensor(v, dtype=torch.int64).reshape(-1) for v in xs]
        yl = [torch.as_tensor(v, dtype=torch.int64).reshape(-1, K) for v in ys]
        xcat = torch.cat(xl).to(self.device).contiguous()
        ycat = torch.cat(yl).to(self.device).contiguous()
        if self.args.special_first:
            ycat = ycat + int(self.args.n_special)
        xo, yo, so, flat, mvals = [0], [0], [0], [], []
        cap = 0
        for b, (xv, yv, mi) in enumerate(zip(xl, yl, mask_intervals)):
            Lx, T = int(xv.numel()), int(yv.shape[0])
            mi = torch.as_tensor(mi, dtype=torch.int64)
            if mi.ndim == 3:
                assert mi.shape[0] == 1 and mi.shape[2] == 2, f"request {b}: mask_interval shape {tuple(mi.shape)}"
                mi = mi[0]
            assert mi.ndim == 2 and mi.shape[1] == 2, f"request {b}: mask_interval shape {tuple(mi.shape)}"
            ivs = [(int(s), int(e)) for s, e in mi.tolist()]
            mvals += self._edit_layout(ivs, T, who=f"request {b}: ")      # shuffle draws in request order
            flat += [v for iv in ivs for v in iv]
            M = len(ivs)
            xo.append(xo[-1] + Lx)
            yo.append(yo[-1] + T)
            so.append(so[-1] + M)
            n_cols = T + 2 * (M + 1) + (M + 1) * K + 1
            cap = max(cap, T + self._gen_budget(Lx, n_cols, 10, spans=M))
        logging.info(f"silence tokens: {list(silence_tokens)}, note that if you are not using the pretrained encodec 6f79c6a8, make sure you specified it yourself, rather than using the default")
        sc = self._sample_cfg(top_k, top_p, temperature, stop_repetition, silence_tokens, _seed, _forced_mode)
        x_off = (C.c_int32 * (B + 1))(*xo)
        y_off = (C.c_int32 * (B + 1))(*yo)
        span_off = (C.c_int32 * (B + 1))(*so)
        iv_arr = (C.c_int32 * max(1, len(flat)))(*flat)
        mv_arr = (C.c_int32 * max(1, len(mvals)))(*mvals)
        res = torch.empty((B, K, cap), dtype=torch.int64, device=self.device)
        res_len = (C.c_int * B)()
        n_steps = C.c_int(0)
        fd, forced_ptr, n_forced = self._forced_arg(_forced, B)
        logits = None
        if _logit_steps > 0:
            V = self.args.audio_vocab_size + int(self.args.n_special)
            logits = torch.zeros((_logit_steps, B, K, V), dtype=torch.float32, device=self.device)
        rc = self.lib.vc_edit_multi(self._h, B, C.c_void_p(xcat.data_ptr()), x_off, C.c_void_p(ycat.data_ptr()), y_off,
                                    iv_arr, span_off, mv_arr, C.byref(sc), forced_ptr, n_forced, C.c_void_p(res.data_ptr()), cap,
                                    res_len, C.c_void_p(logits.data_ptr()) if logits is not None else None, int(_logit_steps),
                                    C.byref(n_steps), self._stream())
        check(rc, self._h, "vc_edit_multi")
        self.last_steps = n_steps.value
        outs = []
        for b in range(B):
            r = res[b, :, : res_len[b]].unsqueeze(0)
            if self.args.special_first:
                r = r - int(self.args.n_special)
            outs.append(r)
        if logits is not None:
            return outs, logits
        return outs

    # ------------------------------------------------------------------ measurement hooks
    def set_option(self, name: str, value) -> None:
        """Run-time launch-shape option of the decode step (include/vc_engine.h vc_set_option), e.g. ("fr_one", "0") or
        ("tile_attn", "2,768").  Exact-mode tokens never depend on one; bf16 logits move by rounding where a form re-orders sums
        (include/vc_engine.h).  bench.py --ab toggles one inside a process."""
        check(self.lib.vc_set_option(self._h, str(name).encode(), str(value).encode()), self._h, f"vc_set_option({name})")

    def options(self) -> str:
        """The engine's option state as text, `key=v,v,...|key=...`: g = graph_steps, nt = (weight mask, K/V loads), fr = finished-row
        forms (finished_rows, fr_pair, att_p16, hq), ta = tile_attn (kernel, min rows), r1 = one-row and attention forms (fr_one,
        attn_fast, qkv_p8), q16 = many-row steps (qkv16, wide_heads, wide_gemm, wd_stage), sh = shrink, w13 = the one-row launches that
        stream their weights as exact 13-bit planes (mask: 1 FFN-down, 4 QKV; w13_stats() says which matrices have planes); an engine
        created with `w8=` appends w8 = the launches that stream E4M3 bytes instead (same bits, w8_stats()), one created with `w8_rows=True`
        w8r = the launches of 2..8-row steps that do (same bits) behind it, one created with `w8_mid=True` w8m = the FFN-down launches of
        9..16-row passes (1, + 8 = also at row counts the measured table leaves out) behind that, one created with `w8_wide=True` w8w = those of 17..64-row
        steps (same bits, + 8 = also at row counts the measured table leaves out) behind that, one created with `w8_up=True` w8u = the
        FFN-up launches of 17..64-row steps (2, 10 = also at row counts the measured table leaves out) behind that, one created with
        `w8_up_rows=True` w8ur = the FFN-up launches of 2..16-row passes (2, 10 likewise) behind that, one created with
        `w8_qkv_rows=True` w8q = the QKV launches of finished-row passes on the 12-channel image (4, 12 likewise) behind that, one created with `kv8=True`
        appends kv8 = decode attention on the E4M3 copy of the K/V cache (1) or on the bf16 cache (0), one created with `kv8="centred"`
        kv8c = 1 behind it.
        bench.py turns it into a JSON object (`config.engine_options`)."""
        return bytes(self.debug_read("options", (256,), torch.uint8).tolist()).split(b"\0")[0].decode()

    def last_timing_ms(self):
        ms = (C.c_float * 3)()
        check(self.lib.vc_last_timing(self._h, ms), self._h, "vc_last_timing")
        return {"prefill_ms": ms[0], "decode_ms": ms[1], "total_ms": ms[2]}

    def bench_kernel(self, which: str, n_rows: int = 1, iters: int = 50):
        ms, nbytes = C.c_float(0), C.c_double(0)
        check(self.lib.vc_bench_kernel(self._h, which.encode(), n_rows, iters, C.byref(ms), C.byref(nbytes), self._stream()),
              self._h, "vc_bench_kernel")
        return ms.value, nbytes.value

    LAUNCH_FORMS = ("rows_gemm", "mt2", "mt4", "blk64", "blk128_sbs", "blk128_2x2", "blk64_occ2", "ln_rows", "rows_attn",
                    "tile_attn", "rows_gemm_fr", "big256", "big128", "row_gemm_fr1", "tile_attn64", "rows_gemm_frp", "wd", "rows_gemm_qp", "w13", "w8",
                    "kv8_attn", "kv8_pack", "kv8c_centre", "kv8c_attn", "kv8c_pack", "w8_rows", "w8_wide", "w8_mid", "w8_up")

    LAUNCH_FORMS_MORE = ("w8_up_rows",)     # the census slots behind LAUNCH_FORMS (vc_debug_read "launch_counts_more")
    LAUNCH_FORMS_MORE2 = ("w8_qkv_rows",)   # ... and behind those (vc_debug_read "launch_counts_more2"): the tuples above are pinned by tests

    def launch_counts(self) -> dict:
        """Process-wide census of the kernel FORMS launched so far (vc_common.h VC_LC_*): the parity tests take the
        difference around a call to assert which form a benchmarked shape really runs on.  w13 / w8 / w8_rows count launches on packed
        weights IN ADDITION to their form's slot: w8 the one-row launches, w8_rows those of 2..8-row steps (rows_gemm_frp / rows_gemm_qp),
        w8_wide those of 17..64-row steps (also in wd), w8_mid the FFN-down launches of 9..16-row passes (also in rows_gemm_fr),
        w8_up the FFN-up launches of 17..64-row steps (also in wd, not in w8_wide), w8_up_rows the FFN-up launches of 2..16-row passes
        (also in rows_gemm), w8_qkv_rows the QKV launches of finished-row passes on the pairs of the 12-channel image (also in
        rows_gemm).  The slots behind LAUNCH_FORMS (LAUNCH_FORMS_MORE, LAUNCH_FORMS_MORE2) are further reads, merged into the same dict."""
        c = self.debug_read("launch_counts", (len(self.LAUNCH_FORMS),), torch.int64)
        out = {n: int(c[i]) for i, n in enumerate(self.LAUNCH_FORMS)}
        m = self.debug_read("launch_counts_more", (len(self.LAUNCH_FORMS_MORE),), torch.int64)
        out.update({n: int(m[i]) for i, n in enumerate(self.LAUNCH_FORMS_MORE)})
        m = self.debug_read("launch_counts_more2", (len(self.LAUNCH_FORMS_MORE2),), torch.int64)
        out.update({n: int(m[i]) for i, n in enumerate(self.LAUNCH_FORMS_MORE2)})
        return out

    W13_MATRICES = ("ffn_down", "qkv")
    W13_STATES = ("not_applicable", "packed", "refused")

    def w13_stats(self) -> list:
        """Per layer, for the matrices of option `w13` (mask bits 1 and 4 in this order): {"state": "packed" | "refused" |
        "not_applicable", "refused_fragments": n}.  A refused matrix holds a 512-value fragment whose non-zero exponents span more than
        30 binades; its launches stay on the bf16 image.  not_applicable: fp32 engine, a width without the form, or VC_W13=0."""
        L = int(self.args.num_decoder_layers)
        v = self.debug_read("w13_stats", (L, 2, 2), torch.int32).tolist()
        return [{m: {"state": self.W13_STATES[v[l][i][0]], "refused_fragments": v[l][i][1]} for i, m in enumerate(self.W13_MATRICES)}
                for l in range(L)]

    W8_MATRICES = ("ffn_down", "qkv")       # mask bits 1 and 4 of option `w8`, the matrices quant.quantize_state_dict_w8 converts
    W8_MASK = 5
    W8_ROWS_MASK = 5                        # option `w8r` of an engine created with w8_rows=True
    W8_MID_MASK = 1                         # option `w8m` of an engine created with w8_mid=True (FFN-down)
    W8_WIDE_MASK = 5                        # option `w8w` of an engine created with w8_wide=True
    W8_UP_MASK = 2                          # option `w8u` of an engine created with w8_up=True (FFN-up)
    W8_UP_ROWS_MASK = 2                     # option `w8ur` of an engine created with w8_up_rows=True (FFN-up)
    W8_QKV_ROWS_MASK = 4                    # option `w8q` of an engine created with w8_qkv_rows=True (QKV)
    # One entry per keyword behind `w8=` (csrc/vc_engine_host.h W8_FORMS): the option it switches on, the request made at creation in
    # this order with the mask of the named class attribute, and where the form packs planes of its own the debug buffer of their
    # per-layer {state, refused pairs} with the w8_stats() key of each matrix in it.
    W8Form = namedtuple("W8Form", "keyword option request mask stats keys")
    W8_FORMS = (
        W8Form("w8_rows", "w8r", "vc_request_w8_rows", "W8_ROWS_MASK", None, ()),
        W8Form("w8_mid", "w8m", "vc_request_w8_mid", "W8_MID_MASK", None, ()),
        W8Form("w8_wide", "w8w", "vc_request_w8_wide", "W8_WIDE_MASK", "w8w_stats", ("ffn_down_wide", "qkv_wide")),
        W8Form("w8_up", "w8u", "vc_request_w8_up", "W8_UP_MASK", "w8u_stats", ("ffn_up_wide",)),
        W8Form("w8_up_rows", "w8ur", "vc_request_w8_up_rows", "W8_UP_ROWS_MASK", "w8ur_stats", ("ffn_up_rows",)),
        W8Form("w8_qkv_rows", "w8q", "vc_request_w8_qkv_rows", "W8_QKV_ROWS_MASK", "w8q_stats", ("qkv_rows",)),
    )

    def w8_stats(self) -> list:
        """w13_stats() for option `w8`: per layer {"ffn_down" | "qkv": {"state": "packed" | "refused" | "not_applicable",
        "refused_fragments": n}}.  A refused matrix holds 512-value fragments off the 8-bit grid; its launches stay where they were.
        not_applicable: an engine created without `w8=`, or a width without the form (FFN-down below d = 512, QKV below d = 1024).
        An engine created with `w8_wide=True` adds "ffn_down_wide" / "qkv_wide": the pair planes of the 16-channel images that 17..64-row
        steps stream, {"state": ..., "refused_pairs": n} (not_applicable: max_seqs <= 16, or a K slice without the form); one created
        with `w8_up=True` adds "ffn_up_wide", the same for the FFN up-projection's image; one created with `w8_up_rows=True` adds
        "ffn_up_rows", the same planes as passes of 2..16 rows see them (not_applicable: a width without the form); one created with
        `w8_qkv_rows=True` adds "qkv_rows", the pairs of the 12-channel QKV image (not_applicable: layer 0, or a width without the form)."""
        L = int(self.args.num_decoder_layers)
        v = self.debug_read("w8_stats", (L, 2, 2), torch.int32).tolist()
        out = [{m: {"state": self.W13_STATES[v[l][i][0]], "refused_fragments": v[l][i][1]} for i, m in enumerate(self.W8_MATRICES)}
               for l in range(L)]
        for form in self.W8_FORMS:
            if form.stats and getattr(self, form.keyword):
                w = self.debug_read(form.stats, (L, len(form.keys), 2), torch.int32).tolist()
                for l in range(L):
                    for i, key in enumerate(form.keys):
                        out[l][key] = {"state": self.W13_STATES[w[l][i][0]], "refused_pairs": w[l][i][1]}
        return out

    def debug_read(self, name: str, shape, dtype=torch.float32) -> torch.Tensor:
        out = torch.empty(shape, dtype=dtype)
        check(self.lib.vc_debug_read(self._h, name.encode(), C.c_void_p(out.data_ptr()), out.numel() * out.element_size()),
              self._h, "vc_debug_read")
        return out


class SessionRequestError(EngineError):
    """Requests of a decode session that finished without a result (DecodeSession.poll / drain): `failed` maps each ticket to the
    exception its fetch raised - EngineError(VC_ECAP) for a request that ran out of max_positions before its terminator,
    AssertionError for one whose x / y held an out-of-range token id.  Their slots are free again; the session goes on, and the
    requests that finished well in the same turn are returned by the next poll() / drain()."""

    def __init__(self, failed: dict):
        self.failed = dict(failed)
        super().__init__("decode session: " + "; ".join(f"ticket {t}: {e}" for t, e in sorted(self.failed.items())))


class DecodeSession:
    """An open decode session of a VoiceCraftEngine (VoiceCraftEngine.open_session).  submit() queues a TTS request, submit_edit()
    an editing request; both return a ticket.  poll() runs one turn of the decode loop and returns the requests that finished;
    drain() polls until the session is idle.  cancel() takes a request out in whatever state it is.  submit(..., stream=True) marks a TTS request as streaming: poll_frames() hands out its
    frames while it decodes, without advancing the loop (voicecraft_amd.stream.SessionStreamer turns them into audio).  While a
    session is open the engine's other decode calls and set_option raise (EngineError, VC_ESTATE)."""

    CONTROLS = ("top_k", "top_p", "temperature", "stop_repetition")

    STATS = ("admitted", "admitted_while_live", "turns", "widenings", "narrowings", "live_rows", "launched_rows", "admission_us")

    def __init__(self, engine: VoiceCraftEngine, max_live: int, sc: SampleCfg, max_samples: int = 1):
        self.engine, self.max_live, self.max_samples = engine, int(max_live), int(max_samples)
        self.kept: dict[int, int] = {}        # ticket -> kept sample index of every best-of-N request fetched so far (submit(n_samples=N))
        self._best_of: set[int] = set()       # unfetched best-of-N tickets
        self._open = False
        self._reqs: dict[int, tuple] = {}     # ticket -> (x, y, T, Lx, M): the device tensors stay alive until the ticket is fetched
                                              # (M: spans of an editing request, 0 = TTS)
        self._sc = sc                         # the session's controls: the default of each field a request does not give
        self._ready: list = []                # (ticket, res, gen) fetched and not yet handed out
        self._streaming: set[int] = set()     # streaming TTS tickets whose last frame has not been pulled (submit(stream=True))
        self._tail: list = []                 # (ticket, first_frame, codes, True): what a finished streaming ticket still had, pulled
                                              # in front of its fetch and handed out by the next poll_frames
        self.cancelled = 0                    # tickets cancelled so far (cancel())
        self._parked: list = []               # [turns left, tensors] of cancelled live tickets: the prefill queued by the turn that admitted
                                              # one may still read its prompt, so the tensors outlive two more turns (or close())
        self.idle = True
        # uploads and result arithmetic run on a stream of the session's own: a launch on the null stream would wait for the decode
        # batches queued on the engine's stream (as in _tts_stream)
        self._side = torch.cuda.Stream(device=engine.device)
        if self.max_samples > 1:
            check(engine.lib.vc_session_open_best_of(engine._h, self.max_live, self.max_samples, C.byref(sc), engine._stream()),
                  engine._h, "vc_session_open_best_of")
        else:
            check(engine.lib.vc_session_open(engine._h, self.max_live, C.byref(sc), engine._stream()), engine._h, "vc_session_open")
        self._open = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def _ctl(self, who: str, controls: dict):
        """The request's vc_request_ctl (None when it gives no control of its own: the session's apply)."""
        bad = sorted(set(controls) - set(self.CONTROLS))
        assert not bad, (f"{who}: {bad} not supported per request - a request's own controls are {list(self.CONTROLS)}; silence_tokens "
                         "and everything else are the session's (open_session)")
        if not controls:
            return None
        ctl = _lib.RequestCtl()
        ctl.top_k = int(controls.get("top_k", self._sc.top_k))
        ctl.top_p = float(controls.get("top_p", self._sc.top_p))
        ctl.temperature = float(controls.get("temperature", self._sc.temperature))
        ctl.stop_repetition = int(controls.get("stop_repetition", self._sc.stop_repetition))
        return ctl

    def _upload(self, x, x_lens, y):
        eng = self.engine
        Lx = int(x_lens[0])                      # (read on the host before anything is queued)
        with torch.cuda.stream(self._side):
            xd, Lx, yd, T = eng._prep(x, torch.tensor([Lx]), y)
        self._side.synchronize()                 # the prompt is on the device before the prefill that reads it can be queued
        return xd, Lx, yd, T

    def submit(self, x, x_lens, y, seed=None, stream: bool = False, n_samples: int = 1, **controls) -> int:
        """A TTS request: x [1,Lx'], x_lens [1], y [1,T,K] as inference_tts takes them (same checks, same special_first handling).
        controls: any of top_k, top_p, temperature, stop_repetition for this request alone; the others are the session's.
        stream=True: the request's frames are handed out by poll_frames() while it decodes (editing requests do not stream:
        submit_edit has no such argument); poll() / drain() return its (ticket, res, gen) as for any other.
        n_samples N > 1 (a session opened with max_samples >= N): a best-of-N request, inference_tts_batch(batch_size=N) on this
        prompt with this seed - N slots, one ticket; the kept sample's (res, gen) comes back and self.kept[ticket] is its index.
        Such a request does not stream (the kept sample is unknown until the group decides); editing requests have no such form."""
        assert self._open, "the session is closed"
        eng = self.engine
        N = int(n_samples)
        assert 1 <= N <= self.max_samples, (f"submit: n_samples {n_samples} outside [1, max_samples = {self.max_samples}] of this "
                                            "session (open_session(max_samples=...))")
        assert not (stream and N > 1), "submit: best-of-N requests do not stream (the kept sample is unknown until the group decides)"
        ctl = self._ctl("submit", controls)
        xd, Lx, yd, T = self._upload(x, x_lens, y)
        sd = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        ticket = C.c_int(0)
        if N > 1:
            check(eng.lib.vc_session_submit_best_of(eng._h, C.c_void_p(xd.data_ptr()), Lx, C.c_void_p(yd.data_ptr()), T, N,
                                                    C.byref(ctl) if ctl is not None else None, sd, C.byref(ticket)),
                  eng._h, "vc_session_submit_best_of")
            self._best_of.add(ticket.value)
        else:
            check(eng.lib.vc_session_submit_ctl(eng._h, C.c_void_p(xd.data_ptr()), Lx, C.c_void_p(yd.data_ptr()), T,
                                                C.byref(ctl) if ctl is not None else None, sd, C.byref(ticket)),
                  eng._h, "vc_session_submit")
        self._reqs[ticket.value] = (xd, yd, T, Lx, 0)
        if stream:
            self._streaming.add(ticket.value)
        self.idle = False
        return ticket.value

    def submit_edit(self, x, x_lens, y, mask_interval, seed=None, _who: str = "", **controls) -> int:
        """An editing request: x, x_lens, y and mask_interval [1,M,2] as `inference` takes them (same checks and messages, the mask
        values derived as there).  controls: as in submit().  A refused request leaves the session running."""
        assert self._open, "the session is closed"
        eng = self.engine
        ctl = self._ctl("submit_edit", controls)
        mask_interval = torch.as_tensor(mask_interval)
        assert mask_interval.ndim == 3 and mask_interval.shape == torch.Size((1, mask_interval.shape[1], 2)), mask_interval
        ivs = [(int(a), int(b)) for a, b in mask_interval[0].tolist()]
        M = len(ivs)
        mask_value = eng._edit_layout(ivs, int(y.shape[1]), who=_who)
        xd, Lx, yd, T = self._upload(x, x_lens, y)
        iv_arr = (C.c_int32 * (2 * M))(*[v for iv in ivs for v in iv])
        mv_arr = (C.c_int32 * (2 * M))(*mask_value)
        sd = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        ticket = C.c_int(0)
        check(eng.lib.vc_session_submit_edit(eng._h, C.c_void_p(xd.data_ptr()), Lx, C.c_void_p(yd.data_ptr()), T, iv_arr, M, mv_arr,
                                             C.byref(ctl) if ctl is not None else None, sd, C.byref(ticket)),
              eng._h, f"{_who}vc_session_submit_edit")
        self._reqs[ticket.value] = (xd, yd, T, Lx, M)
        self.idle = False
        return ticket.value

    def fetch(self, ticket: int):
        """A finished request's result; frees its slot.  A TTS ticket: (res [1,K,T+Tg], gen [1,K,Tg]), the values inference_tts
        returns.  An edit ticket: (res [1,K,T'], None), res being what `inference` returns."""
        assert self._open, "the session is closed"
        eng = self.engine
        K = eng.args.n_codebooks
        req = self._reqs.get(int(ticket))
        xd, yd, T, Lx, M = req if req is not None else (None, None, 0, 1, 0)
        if M:                                    # the buffer of `inference` for this request
            cap = T + eng._gen_budget(Lx, T + 2 * (M + 1) + (M + 1) * K + 1, 10, spans=M)
        else:
            cap = T + eng._gen_budget(Lx, T + 1, eng.args.encodec_sr // 5)
        res = torch.empty((K, cap), dtype=torch.int64, device=eng.device)
        gen_len, n_steps = C.c_int(0), C.c_int(0)
        if int(ticket) in self._best_of:        # the kept sample's index, while the ticket still exists
            k = C.c_int(-1)
            if eng.lib.vc_session_kept(eng._h, int(ticket), C.byref(k)) == 0:
                self.kept[int(ticket)] = int(k.value)
        rc = eng.lib.vc_session_fetch(eng._h, int(ticket), C.c_void_p(res.data_ptr()), cap, C.byref(gen_len), C.byref(n_steps))
        if rc != -2:                           # (an unfinished request keeps its ticket)
            self._reqs.pop(int(ticket), None)
            self._best_of.discard(int(ticket))
        check(rc, eng._h, "vc_session_fetch")
        eng.last_steps = n_steps.value
        if M:                                    # (gen_len is the result length T' of an edit ticket)
            out = res[:, : gen_len.value].unsqueeze(0)
            if eng.args.special_first:
                with torch.cuda.stream(self._side):
                    out = out - int(eng.args.n_special)
                self._side.synchronize()
            return out, None
        Tg = gen_len.value
        out, gen = res[:, : T + Tg].unsqueeze(0), res[:, T: T + Tg].unsqueeze(0)
        if eng.args.special_first:
            with torch.cuda.stream(self._side):
                out, gen = out - int(eng.args.n_special), gen - int(eng.args.n_special)
            self._side.synchronize()             # final on the device: usable from any stream
        return out, gen

    def cancel(self, ticket: int) -> str:
        """Takes a request out of the session: "pending" (it leaves the queue, and whatever waited behind a best-of-N head of the
        line can go in), "live" (its rows are retired by the next turn and its slots come back two turns later, like any
        retirement's) or "finished" (its slot is free at once) says where it was.  The ticket is gone from here on: poll() / drain()
        never return it and poll_frames() has no further chunk for it; chunks already handed out are a prefix of what it would
        have produced.  No partial result comes back.  An unknown, fetched or cancelled ticket raises EngineError; the session
        goes on."""
        assert self._open, "the session is closed"
        eng, t = self.engine, int(ticket)
        if any(r[0] == t for r in self._ready) or any(c[0] == t for c in self._tail):
            # a turn has fetched it already (or pulled its last frames): the engine no longer knows it, drop what waits here
            self._ready = [r for r in self._ready if r[0] != t]
            self._tail = [c for c in self._tail if c[0] != t]
            self.kept.pop(t, None)
            self.cancelled += 1
            return "finished"
        was = C.c_int(-1)
        rc = eng.lib.vc_session_cancel(eng._h, t, C.byref(was))
        if rc == -1:
            msg = eng.lib.vc_last_error(eng._h)
            raise EngineError(f"vc_session_cancel failed (code {rc}): {msg.decode() if msg else ''}")
        check(rc, eng._h, "vc_session_cancel")
        req = self._reqs.pop(t, None)           # at once: poll_frames counts on _reqs listing only possible slot holders, in order
        self._streaming.discard(t)
        self._best_of.discard(t)
        if was.value == 1 and req is not None:
            self._parked.append([2, req])
        self.cancelled += 1
        return ("pending", "live", "finished")[was.value]

    @torch.no_grad()
    def _turn(self) -> None:
        """One turn of the decode loop.  EVERY request it reports finished is fetched: results go to self._ready; if some finished
        without a result, SessionRequestError names them once all are fetched (nothing another request produced is lost)."""
        assert self._open, "the session is closed"
        eng = self.engine
        cap = max(1, self.max_live)
        tickets = (C.c_int * cap)()
        n, idle = C.c_int(0), C.c_int(0)
        check(eng.lib.vc_session_advance(eng._h, tickets, cap, C.byref(n), C.byref(idle)), eng._h, "vc_session_advance")
        self.idle = bool(idle.value)
        self._parked = [[n - 1, req] for n, req in self._parked if n > 1]
        failed = {}
        for i in range(n.value):
            t = int(tickets[i])
            if t in self._streaming:             # what it still has, in front of the fetch that frees its slot: a slow consumer never holds one
                self._tail.append(self._pull_rest(t))
            try:
                self._ready.append((t,) + self.fetch(t))
            except (EngineError, AssertionError) as ex:
                failed[t] = ex
        if failed:
            raise SessionRequestError(failed)

    FRAMES_CAP = 64      # frames per ticket one vc_session_frames call can hand out (what is left comes with the next call)

    def _frames(self, tickets, min_frames: int):
        """One vc_session_frames call: [(ticket, first_frame, codes [1,K,m], done)] of the tickets that got frames or are done."""
        eng = self.engine
        K, n = eng.args.n_codebooks, len(tickets)
        cap = max(int(min_frames), self.FRAMES_CAP)
        buf = torch.empty((n, K, cap), dtype=torch.int64, device=eng.device)
        arr = (C.c_int * n)(*tickets)
        first, cnt, done = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        check(eng.lib.vc_session_frames(eng._h, n, arr, int(min_frames), C.c_void_p(buf.data_ptr()), cap, first, cnt, done),
              eng._h, "vc_session_frames")
        out = [(int(tickets[i]), int(first[i]), buf[i: i + 1, :, : cnt[i]], bool(done[i])) for i in range(n) if cnt[i] or done[i]]
        if eng.args.special_first and any(c.shape[2] for _, _, c, _ in out):
            # not on the null stream: a launch there would wait for the decode batches queued on the engine's stream (as in _tts_stream)
            with torch.cuda.stream(self._side):
                out = [(t, f, c - int(eng.args.n_special), d) for t, f, c, d in out]
            self._side.synchronize()
        return out

    def _pull_rest(self, ticket: int):
        """Everything a finished streaming ticket has not handed out yet, as one last chunk."""
        parts, first = [], None
        while True:
            got = self._frames([ticket], 1)
            assert len(got) <= 1
            for _, f, c, d in got:
                first = f if first is None else first
                parts.append(c)
            if got and got[0][3]:
                break
            assert got, f"ticket {ticket}: reported finished, but its frames are not final"
        self._streaming.discard(ticket)
        if len(parts) > 1:
            with torch.cuda.stream(self._side):
                codes = torch.cat(parts, dim=2)
            self._side.synchronize()
        else:
            codes = parts[0]
        return ticket, first, codes, True

    @torch.no_grad()
    def poll_frames(self, chunk_frames: int = 8):
        """The new frames of the streaming tickets (submit(stream=True)), without advancing the decode loop: a list of (ticket,
        first_frame, codes [1,K,m], done).  Per ticket the chunks are contiguous from frame 0, each of at least `chunk_frames` frames
        except the last, and their concatenation is the `gen` its poll() / drain() entry holds; done comes with the last chunk
        (possibly of 0 frames; at once for a request that ended without a result).  One vc_session_frames call covers every streaming
        ticket that can be holding a slot; what a ticket finished by an earlier poll() still had comes first."""
        assert self._open, "the session is closed"
        assert int(chunk_frames) >= 1, chunk_frames
        out, self._tail = self._tail, []
        # admission is FIFO and a slot is held until its ticket is fetched: only the first max_live unfetched tickets can hold one
        holders = list(self._reqs)[: self.max_live]
        tickets = [t for t in holders if t in self._streaming]
        if tickets:
            got = self._frames(tickets, int(chunk_frames))
            for t, f, c, d in got:
                if d:
                    self._streaming.discard(t)
            out += got
        return out

    def _hand_out(self):
        out, self._ready = self._ready, []
        return out

    def poll(self):
        """One turn of the decode loop; the list of (ticket, res, gen) of the requests that finished since the last call.  Raises
        SessionRequestError (tickets in `.failed`) when a request finished without a result; the others' results are kept and come
        with the next call."""
        self._turn()
        return self._hand_out()

    def drain(self):
        """Polls until the session is idle; everything that finished on the way.  After a SessionRequestError call it again: nothing
        is lost."""
        self._turn()
        while not self.idle:
            self._turn()
        return self._hand_out()

    def stats(self, timing: bool = False) -> dict:
        """The session's counters (include/vc_engine.h vc_session_stats): a function of the submission schedule alone, the same in
        every run of it.  timing=True adds `admission_us`, the decode-stream time spent on admissions so far (HIP events)."""
        assert self._open, "the session is closed"
        v = (C.c_int64 * 8)()
        check(self.engine.lib.vc_session_stats(self.engine._h, v), self.engine._h, "vc_session_stats")
        return {k: int(v[i]) for i, k in enumerate(self.STATS) if timing or k != "admission_us"}

    def close(self) -> None:
        if not self._open:
            return
        self._open = False
        try:
            if self.engine._h:
                check(self.engine.lib.vc_session_close(self.engine._h), self.engine._h, "vc_session_close")
        finally:
            self._reqs.clear()          # the prompts stay valid until the decode stream has been waited for
            self._ready = []
            self._streaming.clear()
            self._best_of.clear()
            self._tail = []
            self._parked = []


def inference_tts_queue(engine: VoiceCraftEngine, xs, ys, max_live: int | None = None, seeds=None, batch_size: int = 1, **sampling):
    """VoiceCraftEngine.inference_tts_queue as a function: any number of utterances through `max_live` slots of one decode session
    (batch_size N > 1: best-of-N per utterance, the kept indices in engine.last_kept)."""
    return engine.inference_tts_queue(xs, ys, max_live=max_live, seeds=seeds, batch_size=batch_size, **sampling)


def inference_queue(engine: VoiceCraftEngine, xs, ys, mask_intervals, max_live: int | None = None, seeds=None, **sampling):
    """VoiceCraftEngine.inference_queue as a function: any number of editing requests through `max_live` slots of one decode session."""
    return engine.inference_queue(xs, ys, mask_intervals, max_live=max_live, seeds=seeds, **sampling)


def debug_sample(logits: torch.Tensor, n_draws: int, top_k: int = -100, top_p: float = 1.0, temperature: float = 1.0,
                 seed: int = 0) -> torch.Tensor:
    """n_draws independent tokens from ONE fp32 logits row [V] on the GPU through the product sampler
    (vc_debug_sample; tests only): int32 [n_draws]."""
    lib = _lib.load()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.ndim == 1
    logits = logits.contiguous()
    sc = SampleCfg()
    sc.top_k, sc.top_p, sc.temperature, sc.seed = int(top_k), float(top_p), float(temperature), int(seed)
    out = torch.empty((n_draws,), dtype=torch.int32, device=logits.device)
    rc = lib.vc_debug_sample(C.c_void_p(logits.data_ptr()), int(logits.numel()), C.byref(sc), int(n_draws),
                             C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream))
    if rc != 0:
        raise AssertionError(f"vc_debug_sample rejected its arguments (code {rc})")
    return out


def debug_attn(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, row_seq: torch.Tensor, row_pos: torch.Tensor,
               n_active: torch.Tensor, share_len: torch.Tensor, nsplit: int, nt: bool = False, fast: bool = True,
               part16: bool = False, x_out: bool = False, sentinel: float = 0.0) -> dict:
    """ONE launch of the decode attention kernel on the caller's tensors (vc_debug_attn; tests only).  q fp32 [rows][H*hd];
    kcache / vcache [n_seqs][H][S_max][hd] fp32 or bf16; row_seq / row_pos int32 [rows]; n_active / share_len int32 [1].
    Returns {"att_o": [rows][H][nsplit][hd] (fp32, bf16 with part16), "att_ml": fp32 [rows][H][nsplit][2]} or, with x_out,
    {"x_out": [rows][H*hd] in the cache dtype}; every output buffer is preset to `sentinel`, so what the launch left unwritten shows."""
    lib = _lib.load()
    dev = q.device
    assert q.is_cuda and q.dtype == torch.float32 and q.ndim == 2 and q.is_contiguous()
    assert kcache.dtype in (torch.float32, torch.bfloat16) and vcache.dtype == kcache.dtype and kcache.shape == vcache.shape
    assert kcache.ndim == 4 and kcache.is_contiguous() and vcache.is_contiguous() and kcache.device == dev == vcache.device
    n_seqs, H, S_max, hd = kcache.shape
    rows = q.shape[0]
    assert q.shape[1] == H * hd
    for t, n in ((row_seq, rows), (row_pos, rows), (n_active, 1), (share_len, 1)):
        assert t.dtype == torch.int32 and t.device == dev and t.numel() == n and t.is_contiguous()
    assert int(row_seq.max()) < n_seqs and int(row_pos.max()) < S_max and int(share_len) <= S_max      # the kernel trusts its tables
    a = _lib.DebugAttnArgs()
    a.q, a.kcache, a.vcache = q.data_ptr(), kcache.data_ptr(), vcache.data_ptr()
    a.row_seq, a.row_pos, a.n_active, a.share_len = row_seq.data_ptr(), row_pos.data_ptr(), n_active.data_ptr(), share_len.data_ptr()
    a.dtype = _lib.VC_DTYPE_BF16 if kcache.dtype == torch.bfloat16 else _lib.VC_DTYPE_F32
    a.H, a.hd, a.S_max, a.rows, a.nsplit = H, hd, S_max, rows, int(nsplit)
    a.nt, a.fast, a.part16 = int(bool(nt)), int(bool(fast)), int(bool(part16))
    out = {}
    if x_out:
        out["x_out"] = torch.full((rows, H * hd), sentinel, dtype=kcache.dtype, device=dev)
        a.x_out = out["x_out"].data_ptr()
    else:
        n = max(int(nsplit), 1)
        out["att_o"] = torch.full((rows, H, n, hd), sentinel, dtype=torch.bfloat16 if part16 else torch.float32, device=dev)
        out["att_ml"] = torch.full((rows, H, n, 2), sentinel, dtype=torch.float32, device=dev)
        a.att_o, a.att_ml = out["att_o"].data_ptr(), out["att_ml"].data_ptr()
    rc = lib.vc_debug_attn(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise AssertionError(f"vc_debug_attn rejected its arguments (code {rc})")
    return out


def debug_tile_attn(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, row_seq: torch.Tensor, row_pos: torch.Tensor,
                    share_len: torch.Tensor, form: int = 1, sentinel: float = 0.0, guard_rows: int = 0) -> torch.Tensor:
    """ONE launch of a prefill attention kernel on the caller's tensors (vc_debug_tile_attn; tests only).  form 1: tile_attn_k, form 2:
    tile_attn64_k.  q fp32 [rows][H*hd]; kcache / vcache [n_seqs][H][S_max][hd] fp32 or bf16; row_seq / row_pos int32 [rows], laid out as
    a prefill pass's (-1 in padding rows); share_len int32 [1].  Returns x_out [rows + guard_rows][H*hd] in the cache dtype, preset to
    `sentinel`: what the launch left unwritten shows, and the guard rows behind the launch's must keep it."""
    lib = _lib.load()
    dev = q.device
    assert q.is_cuda and q.dtype == torch.float32 and q.ndim == 2 and q.is_contiguous()
    assert kcache.dtype in (torch.float32, torch.bfloat16) and vcache.dtype == kcache.dtype and kcache.shape == vcache.shape
    assert kcache.ndim == 4 and kcache.is_contiguous() and vcache.is_contiguous() and kcache.device == dev == vcache.device
    n_seqs, H, S_max, hd = kcache.shape
    rows = q.shape[0]
    assert q.shape[1] == H * hd
    for t, n in ((row_seq, rows), (row_pos, rows), (share_len, 1)):
        assert t.dtype == torch.int32 and t.device == dev and t.numel() == n and t.is_contiguous()
    assert int(row_seq.max()) < n_seqs and int(row_pos.max()) < S_max and 0 <= int(share_len) <= S_max      # the kernels trust their tables
    assert bool(((row_seq >= 0) | (row_pos < 0)).all())
    a = _lib.DebugTileAttnArgs()
    a.q, a.kcache, a.vcache = q.data_ptr(), kcache.data_ptr(), vcache.data_ptr()
    a.row_seq, a.row_pos, a.share_len = row_seq.data_ptr(), row_pos.data_ptr(), share_len.data_ptr()
    a.dtype = _lib.VC_DTYPE_BF16 if kcache.dtype == torch.bfloat16 else _lib.VC_DTYPE_F32
    a.H, a.hd, a.S_max, a.rows, a.form = H, hd, S_max, rows, int(form)
    x = torch.full((rows + int(guard_rows), H * hd), sentinel, dtype=kcache.dtype, device=dev)
    a.x_out = x.data_ptr()
    rc = lib.vc_debug_tile_attn(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise AssertionError(f"vc_debug_tile_attn rejected its arguments (code {rc})")
    return x


def debug_attn8(q, kcache, vcache, kcache8, vcache8, kvshift8, row_seq, row_pos, n_active, share_len, nsplit: int = 1, rps: int = 1,
                pack: bool = False, nt: bool = False, fast: bool = True, part16: bool = False, x_out: bool = False,
                sentinel: float = 0.0) -> dict:
    """vc_debug_attn8 (tests only): debug_attn for option `kv8`.  kcache / vcache bf16 [n_seqs][H][S_max][hd]; kcache8 / vcache8 uint8 of
    that shape; kvshift8 int8 [n_seqs][H][S_max][2].  pack=True: ONE launch of the packer over the rows (row_seq, row_pos), which writes
    the three 8-bit arrays in place ({} comes back).  Else one launch of the decode attention's kv8 form with `rps` rows per sequence;
    the outputs as debug_attn's."""
    lib = _lib.load()
    dev = kcache.device
    assert kcache.dtype == torch.bfloat16 == vcache.dtype and kcache.shape == vcache.shape and kcache.ndim == 4
    n_seqs, H, S_max, hd = kcache.shape
    for t in (kcache8, vcache8):
        assert t.dtype == torch.uint8 and t.shape == kcache.shape
    assert kvshift8.dtype == torch.int8 and tuple(kvshift8.shape) == (n_seqs, H, S_max, 2)
    for t in (kcache, vcache, kcache8, vcache8, kvshift8):
        assert t.is_cuda and t.device == dev and t.is_contiguous()
    rows = row_pos.numel()
    for t, n in ((row_seq, rows), (row_pos, rows), (n_active, 1), (share_len, 1)):
        assert t.dtype == torch.int32 and t.device == dev and t.numel() == n and t.is_contiguous()
    assert int(row_seq.max()) < n_seqs and int(row_pos.max()) < S_max and int(share_len) <= S_max      # the kernels trust their tables
    a8 = _lib.DebugAttn8Args()
    a = a8.base
    a.kcache, a.vcache = kcache.data_ptr(), vcache.data_ptr()
    a8.kcache8, a8.vcache8, a8.kvshift8 = kcache8.data_ptr(), vcache8.data_ptr(), kvshift8.data_ptr()
    a.row_seq, a.row_pos, a.n_active, a.share_len = row_seq.data_ptr(), row_pos.data_ptr(), n_active.data_ptr(), share_len.data_ptr()
    a.dtype = _lib.VC_DTYPE_BF16
    a.H, a.hd, a.S_max, a.rows, a.nsplit = H, hd, S_max, rows, int(nsplit)
    a.nt, a.fast, a.part16 = int(bool(nt)), int(bool(fast)), int(bool(part16))
    a8.rps, a8.pack = int(rps), int(bool(pack))
    out = {}
    if not pack:
        assert q.is_cuda and q.dtype == torch.float32 and q.shape == (rows, H * hd) and q.is_contiguous() and rows % int(rps) == 0
        a.q = q.data_ptr()
        if x_out:
            out["x_out"] = torch.full((rows, H * hd), sentinel, dtype=torch.bfloat16, device=dev)
            a.x_out = out["x_out"].data_ptr()
        else:
            n = max(int(nsplit), 1)
            out["att_o"] = torch.full((rows, H, n, hd), sentinel, dtype=torch.bfloat16 if part16 else torch.float32, device=dev)
            out["att_ml"] = torch.full((rows, H, n, 2), sentinel, dtype=torch.float32, device=dev)
            a.att_o, a.att_ml = out["att_o"].data_ptr(), out["att_ml"].data_ptr()
    rc = lib.vc_debug_attn8(C.byref(a8), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise AssertionError(f"vc_debug_attn8 rejected its arguments (code {rc})")
    return out


def debug_attn8c(q, kcache, vcache, kcache8, vcache8, kvshift8, centre, row_seq, row_pos, n_active, share_len, nsplit: int = 1,
                 rps: int = 1, mode: int = 0, n0=None, nt: bool = False, fast: bool = True, part16: bool = False, x_out: bool = False,
                 sentinel: float = 0.0) -> dict:
    """vc_debug_attn8c (tests only): debug_attn8 for `kv8="centred"`.  centre bf16 [n_seqs][H][hd].  mode 0: one launch of the centred
    attention form (outputs as debug_attn's); mode 1: the centred packer, in place; mode 2: the centre kernel over the rows as a prefill
    pass's, which writes `centre` and n0 (int32 [n_seqs]) in place (the 8-bit arrays, vcache and q may be None)."""
    lib = _lib.load()
    dev = kcache.device
    assert kcache.dtype == torch.bfloat16 and kcache.ndim == 4 and kcache.is_cuda and kcache.is_contiguous()
    n_seqs, H, S_max, hd = kcache.shape
    assert centre.dtype == torch.bfloat16 and tuple(centre.shape) == (n_seqs, H, hd) and centre.device == dev and centre.is_contiguous()
    rows = row_pos.numel()
    for t, n in ((row_seq, rows), (row_pos, rows), (n_active, 1), (share_len, 1)):
        assert t.dtype == torch.int32 and t.device == dev and t.numel() == n and t.is_contiguous()
    assert int(row_seq.max()) < n_seqs and int(row_pos.max()) < S_max and int(share_len) <= S_max      # the kernels trust their tables
    ac = _lib.DebugAttn8cArgs()
    a8 = ac.base8
    a = a8.base
    a.kcache = kcache.data_ptr()
    a.row_seq, a.row_pos, a.n_active, a.share_len = row_seq.data_ptr(), row_pos.data_ptr(), n_active.data_ptr(), share_len.data_ptr()
    a.dtype = _lib.VC_DTYPE_BF16
    a.H, a.hd, a.S_max, a.rows, a.nsplit = H, hd, S_max, rows, int(nsplit)
    a.nt, a.fast, a.part16 = int(bool(nt)), int(bool(fast)), int(bool(part16))
    a8.rps = int(rps)
    ac.centre, ac.mode, ac.n_seqs = centre.data_ptr(), int(mode), n_seqs
    out = {}
    if mode == 2:
        assert n0.dtype == torch.int32 and n0.numel() == n_seqs and n0.device == dev and n0.is_contiguous()
        ac.n0 = n0.data_ptr()
    else:
        assert vcache.dtype == torch.bfloat16 and vcache.shape == kcache.shape
        for t in (kcache8, vcache8):
            assert t.dtype == torch.uint8 and t.shape == kcache.shape
        assert kvshift8.dtype == torch.int8 and tuple(kvshift8.shape) == (n_seqs, H, S_max, 2)
        for t in (vcache, kcache8, vcache8, kvshift8):
            assert t.is_cuda and t.device == dev and t.is_contiguous()
        a.vcache = vcache.data_ptr()
        a8.kcache8, a8.vcache8, a8.kvshift8 = kcache8.data_ptr(), vcache8.data_ptr(), kvshift8.data_ptr()
    if mode == 0:
        assert q.is_cuda and q.dtype == torch.float32 and q.shape == (rows, H * hd) and q.is_contiguous() and rows % int(rps) == 0
        a.q = q.data_ptr()
        if x_out:
            out["x_out"] = torch.full((rows, H * hd), sentinel, dtype=torch.bfloat16, device=dev)
            a.x_out = out["x_out"].data_ptr()
        else:
            n = max(int(nsplit), 1)
            out["att_o"] = torch.full((rows, H, n, hd), sentinel, dtype=torch.bfloat16 if part16 else torch.float32, device=dev)
            out["att_ml"] = torch.full((rows, H, n, 2), sentinel, dtype=torch.float32, device=dev)
            a.att_o, a.att_ml = out["att_o"].data_ptr(), out["att_ml"].data_ptr()
    rc = lib.vc_debug_attn8c(C.byref(ac), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise AssertionError(f"vc_debug_attn8c rejected its arguments (code {rc})")
    return out


def kv8c_quantize_host(rows_bf16: torch.Tensor, centre_bf16: torch.Tensor):
    """csrc/vc_kv8.h's centred encode on the CPU (vc_kv8c_quantize_host): bf16 K rows [..., hd] against ONE centre [hd] ->
    (codes uint8 [..., hd], shift int8 [...])."""
    lib = _lib.load()
    x = rows_bf16.detach().to("cpu", torch.bfloat16).contiguous()
    c = centre_bf16.detach().to("cpu", torch.bfloat16).contiguous()
    hd = x.shape[-1]
    assert tuple(c.shape) == (hd,)
    n = x.numel() // hd
    codes = torch.empty(x.shape, dtype=torch.uint8)
    shift = torch.empty(x.shape[:-1], dtype=torch.int8)
    rc = lib.vc_kv8c_quantize_host(C.c_void_p(x.data_ptr()), C.c_void_p(c.data_ptr()), n, hd, C.c_void_p(codes.data_ptr()),
                                   C.c_void_p(shift.data_ptr()))
    assert rc == 0, rc
    return codes, shift


def kv8_quantize_host(rows_bf16: torch.Tensor):
    """csrc/vc_kv8.h's encode on the CPU (vc_kv8_quantize_host): bf16 rows [..., hd] -> (codes uint8 [..., hd], shift int8 [...])."""
    lib = _lib.load()
    x = rows_bf16.detach().to("cpu", torch.bfloat16).contiguous()
    hd = x.shape[-1]
    n = x.numel() // hd
    codes = torch.empty(x.shape, dtype=torch.uint8)
    shift = torch.empty(x.shape[:-1], dtype=torch.int8)
    rc = lib.vc_kv8_quantize_host(C.c_void_p(x.data_ptr()), n, hd, C.c_void_p(codes.data_ptr()), C.c_void_p(shift.data_ptr()))
    assert rc == 0, rc
    return codes, shift


def box_probe(device="cuda:0", hops: int = 256) -> dict:
    """The box's dependent-load latency as ONE workgroup on an idle chip sees it (vc_box_probe): over a 128 KB ring (cache-resident)
    and a 256 MB ring (memory), plus the shader clock that lone workgroup ran at."""
    lib = _lib.load()
    dev = torch.device(device)
    out = {}
    with torch.cuda.device(dev):
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for name, nbytes in (("l2", 128 << 10), ("hbm", 256 << 20)):
            res = (C.c_float * 2)()
            rc = lib.vc_box_probe(C.c_longlong(nbytes), int(hops), res, s)
            if rc != 0:
                raise EngineError(f"vc_box_probe failed (code {rc})")
            out[f"dependent_load_ns_{name}"] = round(float(res[0]), 1)
            out[f"shader_mhz_{name}_walk"] = round(float(res[1]), 0)
    return out


# ---------------------------------------------------------------------- pattern ops (no engine needed)
def _pattern_call(fn, *args):
    rc = fn(*args)
    if rc != 0:
        raise AssertionError(f"pattern kernel rejected its arguments (code {rc})")


def pattern_shift(z: torch.Tensor, special: int) -> torch.Tensor:
    """z int64 [B,K,T] on the GPU -> [B,K,T+K] (Pattern.build_pattern_sequence values, codebooks_patterns.py:151-176)."""
    lib = _lib.load()
    assert z.is_cuda and z.dtype == torch.int64 and z.ndim == 3
    z = z.contiguous()
    B, K, T = z.shape
    out = torch.empty((B, K, T + K), dtype=torch.int64, device=z.device)
    _pattern_call(lib.vc_pattern_shift, C.c_void_p(z.data_ptr()), B, K, T, int(special), C.c_void_p(out.data_ptr()),
                  C.c_void_p(torch.cuda.current_stream(z.device).cuda_stream))
    return out


def pattern_revert(s: torch.Tensor, T: int, special: int) -> torch.Tensor:
    """s int64 [B,K,S] -> [B,K,T] (Pattern.revert_pattern_sequence values, codebooks_patterns.py:222-245)."""
    lib = _lib.load()
    assert s.is_cuda and s.dtype == torch.int64 and s.ndim == 3
    s = s.contiguous()
    B, K, S = s.shape
    out = torch.empty((B, K, T), dtype=torch.int64, device=s.device)
    _pattern_call(lib.vc_pattern_revert, C.c_void_p(s.data_ptr()), B, K, S, int(T), int(special),
                  C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(s.device).cuda_stream))
    return out


def pattern_unshift(span: torch.Tensor) -> torch.Tensor:
    """span int64 [N,K] (one row per decode step) -> [K,N-K] (models/voicecraft.py:1125-1139)."""
    lib = _lib.load()
    assert span.is_cuda and span.dtype == torch.int64 and span.ndim == 2
    span = span.contiguous()
    N, K = span.shape
    assert N >= K, f"a span has at least K={K} steps, got {N}"      # voicecraft.py:1137
    out = torch.empty((K, N - K), dtype=torch.int64, device=span.device)
    _pattern_call(lib.vc_pattern_unshift, C.c_void_p(span.data_ptr()), N, K, C.c_void_p(out.data_ptr()),
                  C.c_void_p(torch.cuda.current_stream(span.device).cuda_stream))
    return out
