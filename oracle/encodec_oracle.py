"""EnCodec — CPU oracle.  TEST INFRASTRUCTURE ONLY.  **Parity unpinned.**

The reference's codec is audiocraft's EncodecModel (audiocraft @ c5157b5bf14bf83449c17ea1eeb66c19fb4bc7f0,
`README.md:105`, `data/tokenizer.py:109-110`), which is neither vendored in the reference tree nor
installable here, and no reference test pins its outputs.  The restatement used as oracle is the
published `transformers.EncodecModel` implementation (transformers is part of this image), configured to
the VoiceCraft codec shape (16 kHz mono, 64 filters, ratios 8/5/4/2, 2-layer LSTM,
4 x 2048 x 128 RVQ, weight norm, reflect padding, non-causal; 56.8 M parameters).  Which of
use_causal_conv / pad_mode / use_conv_shortcut the real checkpoint used cannot be known from the tree.
"""
from __future__ import annotations

import torch


def build(state_dict: dict[str, torch.Tensor] | None = None, **overrides):
    """overrides: the architecture switches the reference tree does not pin (use_causal_conv, pad_mode,
    use_conv_shortcut, num_residual_layers, dilation_growth_rate), as EncodecConfig names them."""
    from transformers import EncodecConfig, EncodecModel
    kw = dict(target_bandwidths=[2.2], sampling_rate=16000, audio_channels=1, normalize=False,
              chunk_length_s=None, hidden_size=128, num_filters=64, num_residual_layers=1,
              upsampling_ratios=[8, 5, 4, 2], norm_type="weight_norm", kernel_size=7, last_kernel_size=7,
              residual_kernel_size=3, dilation_growth_rate=2, use_causal_conv=False, pad_mode="reflect",
              compress=2, num_lstm_layers=2, trim_right_ratio=1.0, codebook_size=2048, codebook_dim=128,
              use_conv_shortcut=False)
    kw.update(overrides)
    cfg = EncodecConfig(**kw)
    m = EncodecModel(cfg).eval()
    if state_dict is not None:
        missing, unexpected = m.load_state_dict(state_dict, strict=False)
        assert not unexpected, unexpected
        ok = ("stride", "kernel_size", "padding_total", "inited", "cluster_size", "embed_avg")   # buffers without information
        assert all(k.endswith(ok) for k in missing), missing
    return m


def overrides_from_cfg(cfg: dict | None = None) -> dict:
    """The dict `voicecraft_amd.codec.AudioTokenizer` takes (names of `codec.DEFAULT_CFG`; missing keys = the VoiceCraft
    codec shape) as EncodecConfig overrides for `build`.  transformers derives the number of quantizers from
    target_bandwidths[-1], the frame rate and log2(codebook_size): n_q = int(1000 * bw // (frame_rate * bits)) with
    frame_rate = ceil(sampling_rate / hop), so bw = n_q * frame_rate * bits / 1000 (+ half a quantizer of margin against
    rounding) yields n_q.  EncodecModel refuses codebook sizes that are no power of two."""
    import math
    from voicecraft_amd.codec import DEFAULT_CFG
    cf = dict(DEFAULT_CFG, **(cfg or {}))
    size = int(cf["codebook_size"])
    bits = int(math.log2(size))
    assert 2 ** bits == size and bits >= 1, f"EncodecModel needs a power-of-two codebook_size >= 2, not {size}"
    assert int(cf["compress"]) == 2, cf["compress"]
    hop = math.prod(int(r) for r in cf["ratios"])
    frame_rate = math.ceil(int(cf["sample_rate"]) / hop)
    bw = (int(cf["n_q"]) + 0.5) * frame_rate * bits / 1000.0
    return dict(target_bandwidths=[bw], sampling_rate=int(cf["sample_rate"]), hidden_size=int(cf["hidden"]),
                num_filters=int(cf["n_filters"]), upsampling_ratios=[int(r) for r in cf["ratios"]],
                kernel_size=int(cf["kernel_size"]), last_kernel_size=int(cf["last_kernel_size"]),
                residual_kernel_size=int(cf["residual_kernel_size"]), num_lstm_layers=int(cf["lstm_layers"]),
                codebook_size=size, codebook_dim=int(cf["hidden"]), compress=2,
                num_residual_layers=int(cf["num_residual_layers"]), dilation_growth_rate=int(cf["dilation_growth_rate"]),
                use_causal_conv=bool(cf["use_causal_conv"]), pad_mode=cf["pad_mode"],
                use_conv_shortcut=bool(cf["use_conv_shortcut"]))


def build_cfg(state_dict: dict[str, torch.Tensor] | None, cfg: dict | None = None):
    """`build` at the shape of a tokenizer `cfg` dict; checks that the bandwidth gave the wanted number of quantizers."""
    from voicecraft_amd.codec import DEFAULT_CFG
    m = build(state_dict, **overrides_from_cfg(cfg))
    n_q = int(dict(DEFAULT_CFG, **(cfg or {}))["n_q"])
    assert len(m.quantizer.layers) == n_q and m.quantizer.get_num_quantizers_for_bandwidth(None) == n_q, \
        (len(m.quantizer.layers), n_q)
    return m


@torch.no_grad()
def encode(m, wav: torch.Tensor):
    """wav [1,1,N] -> (codes int64 [K,T], latent [T,hidden]), T = ceil(N / hop)"""
    z = m.encoder(wav)                                   # [1,hidden,T]
    codes = m.quantizer.encode(z, None)                  # [K,1,T]
    return codes[:, 0], z[0].transpose(0, 1).contiguous()


@torch.no_grad()
def decode(m, codes: torch.Tensor):
    """codes int64 [K,T] -> wav [hop*T]"""
    q = m.quantizer.decode(codes.unsqueeze(1))           # [1,hidden,T]
    return m.decoder(q)[0, 0]
