"""CPU checks of the fp64 references the op-variant GPU tests rest on (tests/op_refs.py): the rounders agree with torch's / numpy's own
conversions, the codecs invert them, and the tiled single-pass attention model reduces to plain softmax attention without rounding."""
import numpy as np
import torch

import op_refs as R


def _samples():
    g = np.random.default_rng(3)
    x = g.standard_normal(200000) * np.exp2(g.integers(-30, 18, 200000))
    return np.concatenate([x, [0.0, -0.0, 65504.0, 65519.0, 65520.0, 1e6, -1e6, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 57344.0, 6e4]])


def test_rounders_match_library_conversions():
    x = _samples().astype(np.float32)        # torch / numpy convert fp32 sources with one rounding
    xd = x.astype(np.float64)
    assert np.array_equal(R.rne_bf16(xd), torch.from_numpy(x).bfloat16().double().numpy())
    sat = np.clip(xd, -65504.0, 65504.0)     # the kernels saturate; a plain fp16 conversion would give inf
    assert np.array_equal(R.rne_f16(xd), sat.astype(np.float32).astype(np.float16).astype(np.float64))
    e5 = torch.from_numpy(np.clip(x, -57344.0, 57344.0)).to(torch.float8_e5m2).double().numpy()
    assert np.array_equal(R.rne_e5m2(xd), e5)
    assert np.isnan(R.rne_f16(np.array([np.nan]))).all()


def test_codecs_round_trip():
    xd = _samples()
    assert np.array_equal(R.dec_bf16(R.bf16_bits(xd)), R.rne_bf16(xd))
    assert np.array_equal(R.dec_f16(R.f16_bits(xd)), R.rne_f16(xd))
    e5 = R.rne_e5m2(xd)
    assert np.array_equal(R.dec_e5m2((R.f16_bits(e5) >> 8).astype(np.uint8)), e5)   # e5m2 = the upper byte of an fp16


def test_tiled_attention_model_without_rounding_is_softmax():
    g = np.random.default_rng(4)
    q, k, v = g.standard_normal((2, 3, 70, 32)), g.standard_normal((2, 3, 150, 32)), g.standard_normal((2, 3, 150, 32))
    masked = g.random((2, 150)) < 0.3
    masked[:, 0] = False
    bias = g.standard_normal((2, 3, 70, 150))
    exact = R.attention(q, k, v, masked, bias)
    tiled = R.attention(q * 32 ** -0.5 * R.LOG2E, k, v, masked, bias, p_round=lambda p: p)
    assert np.abs(tiled - exact).max() < 1e-12
