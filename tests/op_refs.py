"""Plain fp64 references and bit-level codecs shared by the op-level parity tests (numpy only, no GPU).

Rounders return float64 arrays holding values of the target format (round to nearest, ties to even); decoders turn the raw 16-bit /
8-bit patterns a kernel wrote back into float64.  The 16-bit / 8-bit layouts are the ones of ec_common.h: bf16 = the upper half of an
fp32, e5m2 = the upper byte of an IEEE fp16, an fp16x2 row = [n x fp16 | n x e5m2 of (v - hi) * 2^11 | n x e5m2 of v]."""
import numpy as np

LOG2E = 1.44269504088896340736


def _rne(x, p, emin):
    """Round float64 x to p significand bits with normal exponents >= emin (subnormals below), ties to even; no overflow handling."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)                                   # x = m 2^e, 0.5 <= |m| < 1: x in [2^(e-1), 2^e)
    q = np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))
    with np.errstate(invalid="ignore"):
        return np.round(x / q) * q                        # x / q is exact (power of two); np.round rounds halves to even


def rne_bf16(x):
    return _rne(x, 8, -126)


def rne_f16(x):
    """IEEE fp16, saturated at +-65504 as the kernels' conversions are (ec_common.h sat_h16); NaN stays NaN."""
    return np.clip(_rne(x, 11, -14), -65504.0, 65504.0)


def rne_e5m2(x):
    """e5m2 (fp16's exponent range, 2 stored mantissa bits), clamped at +-57344 first as pack4_e5m2 does."""
    return _rne(np.clip(x, -57344.0, 57344.0), 3, -14)


def ulp(x, p, emin):
    """Spacing of the p-bit format at |x| (the binade of x, floored at the subnormal spacing)."""
    _, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))


def bf16_bits(x):
    """float array -> uint16 bf16 patterns, RNE (the values of rne_bf16 are exact fp32 values)."""
    return (rne_bf16(x).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def f16_bits(x):
    return rne_f16(x).astype(np.float16).view(np.uint16)


def dec_bf16(u16):
    return (np.asarray(u16, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def dec_f16(u16):
    return np.asarray(u16, np.uint16).view(np.float16).astype(np.float64)


def dec_e5m2(u8):
    return dec_f16(np.asarray(u8, np.uint8).astype(np.uint16) << 8)


def dec_split_bf16(rows, n):
    """bf16 split rows [n hi | n lo] (uint16 [..., >= 2n]) -> (hi, lo) float64."""
    return dec_bf16(rows[..., :n]), dec_bf16(rows[..., n:2 * n])


def dec_x2(rows, n):
    """fp16x2 rows (uint16 [..., >= 2n]: n fp16, then 2n bytes) -> (hi, lo8 / 2^11, hi8) float64, decoded as the GEMM that reads them."""
    rows = np.ascontiguousarray(rows[..., :2 * n])
    b = rows.view(np.uint8)
    return dec_f16(rows[..., :n]), dec_e5m2(b[..., 2 * n:3 * n]) / 2048.0, dec_e5m2(b[..., 3 * n:4 * n])


def attention(q, k, v, masked=None, bias=None, p_round=None, tile=64):
    """softmax(q k^T hd^-0.5 + bias, masked keys removed) v in fp64, per (batch, head): q [B,H,Lq,hd], k / v [B,H,Lk,hd],
    masked [B,Lk] bool or None, bias [B,H,Lq,Lk] or None.

    p_round=None: the exact operation.  p_round=f: the kernel's form with rounded probabilities - the scores are taken in the exp2
    domain (q must then be the kernel's pre-scaled Q, q * hd^-0.5 * log2(e), as the kernel rounded it), keys are visited in tiles of
    `tile` with a running maximum m_t per query, P = f(exp2(s - m_t)) is what multiplies V, the tile's contribution is rescaled by
    exp2(m_t - m_final), and the normaliser is the sum of the UNROUNDED exp2(s - m_final)."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    hd, Lk = q.shape[-1], k.shape[-2]
    if p_round is None:
        s = q @ np.swapaxes(k, -1, -2) * hd ** -0.5
        if bias is not None:
            s = s + bias
    else:
        s = q @ np.swapaxes(k, -1, -2)
        if bias is not None:
            s = s + bias * LOG2E
    if masked is not None:
        s = np.where(np.asarray(masked, bool)[:, None, None, :], -np.inf, s)
    m = s.max(-1, keepdims=True)
    if p_round is None:
        e = np.exp(s - m)
        return (e @ v) / e.sum(-1, keepdims=True)
    nt = -(-Lk // tile)
    pad = np.full(s.shape[:-1] + (nt * tile - Lk,), -np.inf)
    tmax = np.concatenate([s, pad], -1).reshape(s.shape[:-1] + (nt, tile)).max(-1)
    mt = np.maximum(np.maximum.accumulate(tmax, -1), -1e30)         # the kernel's running maximum starts at -1e30
    mk = np.repeat(mt, tile, -1)[..., :Lk]
    with np.errstate(invalid="ignore"):
        pk = p_round(np.exp2(s - mk)) * np.exp2(mk - m)
    return (pk @ v) / np.exp2(s - m).sum(-1, keepdims=True)


def layernorm(x, w, b, eps):
    """Row LayerNorm in fp64 (biased variance, as torch): returns (y, xhat, rstd [rows, 1])."""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps)
    xhat = (x - mu) * rstd
    return xhat * np.asarray(w, np.float64) + np.asarray(b, np.float64), xhat, rstd
