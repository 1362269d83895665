"""-m gpu: every attention and LayerNorm form the model launches, op by op (ec_op_attention_ex / ec_op_layernorm_ex), against fp64.

Each case lays its operands out as the model does (interleaved Q|K|V rows, K|V rows, sliced heads, mask windows, wide batch strides,
fused residual branches, dropped cls rows) and checks, besides the values:
  * poison: every allocated element the kernel must not read is NaN (slack columns, rows past Lk, the gap of the wide K|V layout, the
    tail after the last batch), every element it must not write holds a sentinel (rows past Lq / past the output rows, slack columns);
    the output must be finite and the sentinels unchanged.  Nothing is ever read or written outside the buffers allocated here.
  * determinism: a second launch gives the same bits.
References and rounders: tests/op_refs.py."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import op_refs as R

pytestmark = pytest.mark.gpu

EC_F32, EC_BF16, EC_BF16X3, EC_F16, EC_MIXED, EC_F16X2 = 0, 1, 2, 3, 4, 5
NAN16 = 0x7FFF                      # a NaN in bf16 and in fp16
SENT16, SENT32 = 0x5A5A, 0x7F80DEAD  # output sentinels (raw patterns; compared bit for bit)
G_SPLIT = 1e-4                       # bf16x3 class (tests/test_gpu_ops.py test_attention_bf16x3)
# single-pass fp16 (EC_MIXED) against the fp64 model of the kernel's own roundings (op_refs.attention with p_round): what is left is
# fp32 accumulation of the scores and of O, v_exp_f32 and the fp16 ties they move.  A flipped P moves O by one fp16 ulp of that P times
# v / l: up to 2^-11 * 4.5 ~ 2.2e-3 for a second key near P = 1 with l ~ 1 (the biased self-attention), 4e-4 seen - the max gate
# bounds those; the MEAN gate is the tight one, and it is the one that separates fp16 P from bf16 P (> 7x, asserted per case)
G_ONE_MAX, G_ONE_MEAN = 1.5e-3, 2e-5


@pytest.fixture(scope="module")
def lib():
    from edgecape_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _chk(lib, rc):
    assert rc == 0, lib.ec_last_error().decode()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _dev(a):
    """host array -> device tensor with the same bytes (uint16 / uint32 patterns travel as int16 / int32)"""
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint16, np.uint32):
        a = a.view(np.int16 if a.dtype == np.uint16 else np.int32)
    return torch.from_numpy(a).cuda()


def _host(t, dt):
    return t.cpu().numpy().view(dt)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
class Operand:
    """A [B, L, H*hd] operand placed at column `col` of rows of stride `ld`, batch stride `s`, in a flat buffer of `dt` (np.float32 or
    np.uint16 bit patterns) whose every other element is poison; `tail` extra elements after the last batch."""

    def __init__(self, B, L, width, ld, s, col=0, dt=np.float32, tail=None):
        self.B, self.L, self.width, self.ld, self.s, self.col, self.dt = B, L, width, ld, s, col, dt
        self.n = (B - 1) * s + L * ld + (tail if tail is not None else 64 * ld)

    def index(self):
        b, l, c = np.meshgrid(np.arange(self.B), np.arange(self.L), np.arange(self.width), indexing="ij")
        return b * self.s + l * self.ld + self.col + c


def _fill(n, dt, poison):
    return np.full(n, poison, dt) if dt == np.uint16 else np.full(n, np.nan, np.float32)


def _put(buf, op, vals, kind):
    """vals [B, L, width] float64 of values already in the storage format; kind 'f32' / 'bf16' / 'f16'."""
    enc = {"f32": lambda x: x.astype(np.float32), "bf16": R.bf16_bits, "f16": R.f16_bits}[kind]
    buf[op.index()] = enc(vals)


def _heads(x, H):   # [B, L, H*hd] -> [B, H, L, hd]
    B, L, W = x.shape
    return x.reshape(B, L, H, W // H).transpose(0, 2, 1, 3)


def _round(kind):
    return {"f32": lambda x: x.astype(np.float32).astype(np.float64), "bf16": R.rne_bf16, "f16": R.rne_f16}[kind]


@functools.lru_cache(maxsize=None)
def _data(site, shape, kind):
    """Operand values (float64, already in `kind`'s format) and masks / bias of one call site, shared by every form using them."""
    g = _rng(site, shape)
    r = _round(kind)
    if site == "backbone":
        H, T, B = shape
        C = H * 64
        x = g.standard_normal((B, T, 3 * C))
        return dict(q=r(x[..., :C]), k=r(x[..., C:2 * C]), v=r(x[..., 2 * C:]), masked=None, bias=None)
    if site == "encoder":   # image tokens then K keypoint tokens; only the keypoint keys are masked (window start HW, length K)
        HW, K, B, d = shape[0], 100, 2, 256
        x = g.standard_normal((B, HW + K, 3 * d)) * 1.5
        km = (g.random((B, K)) < 0.4).astype(np.uint8)
        km[0, 0] = km[0, K - 1] = 1          # first and last key of the window masked in sample 0 ...
        km[1, 0] = km[1, K - 1] = 0          # ... visible in sample 1
        masked = np.concatenate([np.zeros((B, HW), bool), km.astype(bool)], 1)
        return dict(q=r(x[..., :d]), k=r(x[..., d:2 * d]), v=r(x[..., 2 * d:]), masked=masked, kmask=km, bias=None)
    if site == "selfattn":   # decoder / skeleton self-attention: B = 3 bs samples share bs mask rows (mask_mod = bs)
        K, bs, d = 100, 2, 256
        B = 3 * bs
        x = g.standard_normal((B, K, 3 * d)) * 1.5
        km = (g.random((bs, K)) < 0.4).astype(np.uint8)
        km[0, 0] = 0
        km[1, :] = 1
        km[1, 0] = 0                          # a sample without a valid keypoint: only key 0 visible (adj_build's kmask_fixed)
        bias = g.standard_normal((B, 8, K, K)) * 2.0
        return dict(q=r(x[..., :d]), k=r(x[..., d:2 * d]), v=r(x[..., 2 * d:]), masked=km.astype(bool)[np.arange(B) % bs], kmask=km,
                    bias=bias)
    if site in ("t2i", "i2t"):   # token -> image (Lq = K, Lk = HW) / image -> token (Lq = HW, Lk = K); E = 512, 8 heads of 64
        HW, K, B, E = shape[0], 100, 2, 512
        Lq, Lk = (K, HW) if site == "t2i" else (HW, K)
        q = g.standard_normal((B, Lq, E)) * 1.5
        kv = g.standard_normal((B, Lk, 2 * E))
        rk = R.rne_f16 if kind == "f16" else _round("f32")     # kind f16: fp16 K|V (kv16), Q stays fp32
        return dict(q=_round("f32")(q), k=rk(kv[..., :E] * 1.5), v=rk(kv[..., E:]), masked=None, bias=None)
    raise AssertionError(site)


def _scaled_q(q, hd, rnd):
    """The kernel's pre-scaled Q (fp32 q * fp32(hd^-0.5 * log2 e)), rounded as the single-pass form rounds it."""
    sc = np.float32(np.float32(1.0 / np.sqrt(hd)) * np.float32(R.LOG2E))
    return rnd((q.astype(np.float32) * sc).astype(np.float64))


@functools.lru_cache(maxsize=None)
def _ref(site, shape, kind, form, H):
    """fp64 reference [B, Lq, H*hd] of one site / operand kind; form 'one' / 'one_bf16P' model the single-pass fp16 roundings."""
    d = _data(site, shape, kind)
    q, k, v = (_heads(d[n], H) for n in ("q", "k", "v"))
    if form == "exact":
        o = R.attention(q, k, v, d["masked"], d["bias"])
    else:
        hd = q.shape[-1]
        pr = R.rne_f16 if form == "one" else R.rne_bf16
        o = R.attention(_scaled_q(q, hd, R.rne_f16), R.rne_f16(k), R.rne_f16(v), d["masked"], d["bias"], p_round=pr)
    B, _, Lq, hd = o.shape
    return o.transpose(0, 2, 1, 3).reshape(B, Lq, H * hd)


def _launch(lib, bufs, O, o_host, mode, kv16, o_x3, a):
    """Two launches on fresh copies of the output buffer; returns the first result (host), asserting the second is bit-identical."""
    outs = []
    for _ in range(2):
        od = _dev(o_host)
        _chk(lib, lib.ec_op_attention_ex(_p(bufs["q"]), _p(bufs["k"]), _p(bufs["v"]), _p(od), a["ldq"], a["ldk"], a["ldv"], O.ld,
                                          a["sQ"], a["sK"], a["sV"], O.s, _p(bufs.get("kmask")), a.get("mask_start", 0),
                                          a.get("mask_len", 0), a.get("mask_mod", 0), _p(bufs.get("bias")), a["B"], a["H"], a["Lq"],
                                          a["Lk"], a["hd"], mode, kv16, o_x3, None))
        torch.cuda.synchronize()
        outs.append(_host(od, o_host.dtype))
    assert np.array_equal(outs[0].view(np.uint8), outs[1].view(np.uint8)), "second launch differs"
    return outs[0]


def _check_sentinels(out, O, written_width):
    keep = np.ones(O.n, bool)
    b, l, c = np.meshgrid(np.arange(O.B), np.arange(O.L), np.arange(written_width), indexing="ij")
    keep[(b * O.s + l * O.ld + c).ravel()] = False
    sent = SENT16 if O.dt == np.uint16 else SENT32
    raw = out.view(np.uint16 if O.dt == np.uint16 else np.uint32)
    assert np.all(raw[keep] == sent), f"{int((raw[keep] != sent).sum())} elements written outside the output"


def _run_site(lib, site, shape, form, kv16=0, o_x3=0, wide=False):
    """Lay out one call site as the model does, launch it, return (decoded output [B, Lq, C] float64 (+ planes), the reference key)."""
    if site == "backbone":
        H, T, B = shape
        C, hd, Lq, Lk = H * 64, 64, T, T
        kind = {"bf16": "bf16", "f16": "f16"}.get(form, "f32")
        dt = np.uint16 if kind != "f32" else np.float32
        d = _data(site, shape, kind)
        ops = {n: Operand(B, T, C, 3 * C, T * 3 * C, i * C, dt) for i, n in enumerate("qkv")}   # interleaved Q|K|V, ld = 3C
        buf = _fill(ops["q"].n, dt, NAN16)
        for n in "qkv":
            _put(buf, ops[n], d[n], kind)
        qkv = _dev(buf)
        es = 2 if dt == np.uint16 else 4
        bufs = {"q": qkv, "k": _Off(qkv, C * es), "v": _Off(qkv, 2 * C * es)}
        ldq = 3 * C
        a = dict(ldq=ldq, ldk=ldq, ldv=ldq, sQ=T * ldq, sK=T * ldq, sV=T * ldq, B=B, H=H, Lq=Lq, Lk=Lk, hd=hd)
        mode = {"bf16": EC_BF16, "f16": EC_F16}.get(form, EC_BF16X3)
        owidth = 2 * C if o_x3 else C
        O = Operand(B, Lq, owidth, owidth, T * owidth, 0, np.uint16 if (kind != "f32" or o_x3) else np.float32)
    else:
        if site in ("encoder", "selfattn"):
            H, hd, d = 8, 32, 256
            L = shape[0] + 100 if site == "encoder" else 100
            B = 2 if site == "encoder" else 6
            kind = "f32"
            dd = _data(site, shape, kind)
            ops = {n: Operand(B, L, d, 3 * d, L * 3 * d, i * d) for i, n in enumerate("qkv")}
            buf = _fill(ops["q"].n, np.float32, 0)
            for n in "qkv":
                _put(buf, ops[n], dd[n], kind)
            qkv = _dev(buf)
            bufs = {"q": qkv, "k": _Off(qkv, d * 4), "v": _Off(qkv, 2 * d * 4), "kmask": _dev(dd["kmask"])}
            a = dict(ldq=3 * d, ldk=3 * d, ldv=3 * d, sQ=L * 3 * d, sK=L * 3 * d, sV=L * 3 * d, B=B, H=H, Lq=L, Lk=L, hd=hd,
                     mask_len=100)
            if site == "encoder":
                a["mask_start"] = shape[0]
            else:
                a["mask_mod"] = 2
                bufs["bias"] = _dev(dd["bias"].astype(np.float32))
            O = Operand(B, L, d, d, L * d)
        else:
            HW, K, B, E, H, hd = shape[0], 100, 2, 512, 8, 64
            Lq, Lk = (K, HW) if site == "t2i" else (HW, K)
            kind = "f16" if kv16 else "f32"
            dd = _data(site, shape, kind)
            Q = Operand(B, Lq, E, E, Lq * E)
            qb = _fill(Q.n, np.float32, 0)
            _put(qb, Q, dd["q"], "f32")
            kvdt = np.uint16 if kv16 else np.float32
            sKV = (HW + K) * 2 * E if wide else Lk * 2 * E        # wide: sample b's image rows start at row b (HW + K)
            ops = {n: Operand(B, Lk, E, 2 * E, sKV, i * E, kvdt) for i, n in enumerate("kv")}
            kvb = _fill(ops["k"].n, kvdt, NAN16)
            for n in "kv":
                _put(kvb, ops[n], dd[n], kind)
            kvt = _dev(kvb)
            bufs = {"q": _dev(qb), "k": kvt, "v": _Off(kvt, E * (2 if kv16 else 4))}
            a = dict(ldq=E, ldk=2 * E, ldv=2 * E, sQ=Lq * E, sK=sKV, sV=sKV, B=B, H=H, Lq=Lq, Lk=Lk, hd=hd)
            O = Operand(B, Lq, E, E, Lq * E)
        mode = EC_MIXED if form.startswith("one") else EC_BF16X3
        owidth = O.width
    o_host = np.full(O.n, SENT16 if O.dt == np.uint16 else SENT32, np.uint16 if O.dt == np.uint16 else np.uint32)
    if O.dt == np.float32:
        o_host = o_host.view(np.float32)
    out = _launch(lib, bufs, O, o_host, mode, kv16, o_x3, a)
    _check_sentinels(out, O, owidth)
    return out[O.index()]      # [B, Lq, owidth]


class _Off:
    """A device pointer `off` bytes into a tensor (the K / V slices of an interleaved buffer)."""

    def __init__(self, t, off):
        self.t, self.off = t, off

    def data_ptr(self):
        return self.t.data_ptr() + self.off


def _assert_close(got, ref, gmax, gmean=None):
    assert np.isfinite(got).all(), "non-finite output"
    err = np.abs(got - ref)
    assert err.max() < gmax and (gmean is None or err.mean() < gmean), (float(err.max()), gmax, float(err.mean()), gmean)


def _check_one(got, site, shape, kind, H):
    """Single-pass fp16 output against the fp64 model of its roundings, and proof that the gate tells fp16 P from bf16 P."""
    ref = _ref(site, shape, kind, "one", H)
    alt = _ref(site, shape, kind, "one_bf16P", H)
    assert np.abs(alt - ref).mean() > 2 * G_ONE_MEAN, float(np.abs(alt - ref).mean())     # the mean gate separates the two models
    _assert_close(got, ref, G_ONE_MAX, G_ONE_MEAN)


BACKBONE = {"vits224": (6, 257, 2), "vitb256": (12, 325, 2), "vitl384": (16, 730, 1), "s224x308": (6, 353, 2)}


@pytest.mark.parametrize("form", ["bf16", "f16", "x3_0", "x3_1", "x3_3"])
@pytest.mark.parametrize("shape", list(BACKBONE))
def test_attn_backbone(lib, shape, form):
    """Backbone self-attention on the interleaved Q|K|V rows (ld = 3C) the QKV GEMM writes: the 16-bit kernels in place (the buffer
    descriptor that ends with key row Lk - 1 meets NaN rows right after the last image), and the split kernel with fp32 O, bf16
    [hi | lo] O (bf16x3 backbone) and fp16x2 O (fp16x2 backbone), ldo = 2C for the last two."""
    H, T, B = BACKBONE[shape]
    C = H * 64
    o_x3 = int(form[-1]) if form.startswith("x3") else 0
    got = _run_site(lib, "backbone", BACKBONE[shape], form, o_x3=o_x3)
    if form in ("bf16", "f16"):
        ref = _ref("backbone", BACKBONE[shape], form, "exact", H)
        dec = R.dec_bf16 if form == "bf16" else R.dec_f16
        gmax, gmean = (2e-2, 2e-3) if form == "bf16" else (3e-3, 3e-4)   # test_gpu_ops.py test_attention_bf16 / _fp16
        _assert_close(dec(got), ref, gmax, gmean)
        return
    ref = _ref("backbone", BACKBONE[shape], "f32", "exact", H)
    if o_x3 == 0:
        _assert_close(got.astype(np.float64), ref, G_SPLIT)
    elif o_x3 == 1:
        hi, lo = R.dec_split_bf16(got, C)
        _assert_close(hi + lo, ref, G_SPLIT)
        assert np.all(np.abs(hi - ref) <= np.abs(ref) * 2.0 ** -8 + G_SPLIT), "bf16 hi plane beyond half an ulp"
    else:
        hi, lo8, hi8 = R.dec_x2(got, C)
        assert np.isfinite(hi).all() and np.isfinite(hi8).all()
        # lo = v - hi is within half an fp16 ulp of v (2^-11 |v|); its e5m2 copy keeps 3 significand bits: half an ulp of it is 2^-14 |v|
        assert np.all(np.abs(hi + lo8 - ref) <= G_SPLIT + np.abs(ref) * 2.0 ** -14), float(np.abs(hi + lo8 - ref).max())
        assert np.all(np.abs(hi - ref) <= np.abs(ref) * 2.0 ** -11 + G_SPLIT), "fp16 plane beyond half an ulp"
        assert np.all(np.abs(hi8 - ref) <= np.abs(ref) * 2.0 ** -3 + G_SPLIT + 2.0 ** -17), "e5m2 hi8 plane beyond half an ulp"


HWS = {"hw256": 256, "hw324": 324, "hw729": 729, "hw14x20": 280}


@pytest.mark.parametrize("hw", list(HWS))
def test_attn_encoder_window(lib, hw):
    """Head encoder: L = HW + K tokens, interleaved Q|K|V (ld = 3d), key mask window starting at HW (image keys never masked), with
    the window's first and last key masked in one sample and visible in the other."""
    shape = (HWS[hw],)
    got = _run_site(lib, "encoder", shape, "split")
    _assert_close(got.astype(np.float64), _ref("encoder", shape, "f32", "exact", 8), G_SPLIT)


@pytest.mark.parametrize("form", ["split", "one"])
def test_attn_selfattn_bias_maskmod(lib, form):
    """Decoder / skeleton self-attention: biased ([B,H,K,K]), mask rows shared by sample % bs (B = 3 bs), one sample whose only
    visible key is key 0; bf16x3 and the mixed head's single-pass fp16 form."""
    shape = (100,)
    got = _run_site(lib, "selfattn", shape, form).astype(np.float64)
    if form == "split":
        _assert_close(got, _ref("selfattn", shape, "f32", "exact", 8), G_SPLIT)
    else:
        _check_one(got, "selfattn", shape, "f32", 8)


@pytest.mark.parametrize("variant", ["split", "split_kv16", "split_kv16_wide", "one", "one_kv16", "one_kv16_wide"])
@pytest.mark.parametrize("hw", list(HWS))
def test_attn_token_to_image(lib, hw, variant):
    """Token -> image cross attention: Q rows of E, K|V rows of 2E (fp32, or fp16 from the image projection with kv16); `wide`: the
    batch stride of the all-rows projection, (HW + K) 2E, with NaN rows in the gap past Lk."""
    shape = (HWS[hw],)
    kv16 = 1 if "kv16" in variant else 0
    got = _run_site(lib, "t2i", shape, variant, kv16=kv16, wide="wide" in variant).astype(np.float64)
    kind = "f16" if kv16 else "f32"
    if variant.startswith("split"):
        _assert_close(got, _ref("t2i", shape, kind, "exact", 8), G_SPLIT)
    else:
        _check_one(got, "t2i", shape, kind, 8)


@pytest.mark.parametrize("form", ["split", "one"])
@pytest.mark.parametrize("hw", list(HWS))
def test_attn_image_to_token(lib, hw, form):
    """Image -> token attention of the two-way layers: Lq = HW image queries over the K keypoint keys of K|V rows of 2E."""
    shape = (HWS[hw],)
    got = _run_site(lib, "i2t", shape, form).astype(np.float64)
    if form == "split":
        _assert_close(got, _ref("i2t", shape, "f32", "exact", 8), G_SPLIT)
    else:
        _check_one(got, "i2t", shape, "f32", 8)


def test_attn_unimplemented_precision_is_an_error(lib):
    """ec_op_attention(EC_MIXED) and ec_op_linear(EC_F16X2) used to run the fp32 kernels silently; they are argument errors."""
    B, H, L, hd = 1, 2, 64, 32
    q = torch.randn(B, L, H * hd, device="cuda")
    o = torch.empty_like(q)
    rc = lib.ec_op_attention(_p(q), _p(q), _p(q), None, None, _p(o), B, H, L, L, hd, EC_MIXED, None)
    assert rc == -1 and b"precision" in lib.ec_last_error()
    A, W, Cm = torch.randn(128, 128, device="cuda"), torch.randn(128, 128, device="cuda"), torch.empty(128, 128, device="cuda")
    rc = lib.ec_op_linear(_p(A), _p(W), None, None, None, _p(Cm), 128, 128, 128, 0, EC_F16X2, None)
    assert rc == -1 and b"precision" in lib.ec_last_error()
    rc = lib.ec_op_attention_ex(_p(q), _p(q), _p(q), _p(o), H * hd, H * hd, H * hd, H * hd, L * H * hd, L * H * hd, L * H * hd,
                                L * H * hd, None, 0, 0, 0, None, B, H, L, L, hd, EC_F16X2, 0, 0, None)
    assert rc == -1 and b"mode" in lib.ec_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24          # fp32 unit roundoff
EPS = 1e-6


def ln_gate(x, w, b, xhat, rstd):
    """Bound on |fp32 kernel - fp64 LayerNorm| per element, from layernorm_kernel's arithmetic (ec_ops.hip):
      * row sums: every element passes through at most D = 14 fp32 additions (3 inside its float4, 4 into the lane's sum, 6 butterfly
        levels of wave_sum) and one division by cols, each rounding by at most U times the partial sum, so the mean is off by at most
        D U mean|x|; that shift reaches the output as |w| rstd D U mean|x| - the term that dominates on rows with a large common offset;
      * the variance sum of d^2 (positive terms) is off by (D + 3) U relative, its rsqrt by half that plus ~2 U for the division / eps /
        v_rsq_f32: ~11 U on rstd; (x - mean) rstd w + b adds three roundings - together <= 16 U (|w xhat| + |b|).
    On unit-scale Gaussian rows this is ~1e-6 for typical elements and reaches 2e-5 only at |w xhat| ~ 20."""
    D = 14
    return 16 * U * (np.abs(w * xhat) + np.abs(b)) + np.abs(w) * rstd * D * U * np.abs(x).mean(-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _ln_data(rows, cols):
    """Rows cycle through three kinds: 0 Gaussian, 1 a large common offset (1000 + N(0, 1)), 2 one planted outlier channel at 500x the
    median magnitude (the residual-stream pattern of DINOv2)."""
    g = _rng("ln", rows, cols)
    x = g.standard_normal((rows, cols))
    kind = np.arange(rows) % 3
    x[kind == 1] += 1000.0
    med = np.median(np.abs(x[kind == 2]), -1) if (kind == 2).any() else 0
    x[kind == 2, 7 % cols] = 500.0 * med
    x = x.astype(np.float32).astype(np.float64)
    w = (g.standard_normal(cols)).astype(np.float32).astype(np.float64)
    b = (g.standard_normal(cols)).astype(np.float32).astype(np.float64)
    return x, w, b, kind


def _ln_ref(x, w, b):
    y, xhat, rstd = R.layernorm(x, w, b, EPS)
    return y, ln_gate(x, w, b, xhat, rstd)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class Rows:
    """rows x width elements of stride ld (dt float32 / uint16) plus `tail` rows, everything else filled with `fill`."""

    def __init__(self, rows, width, ld, dt, fill, tail=4):
        self.rows, self.width, self.ld, self.dt = rows, width, ld, dt
        self.buf = np.full((rows + tail) * ld, fill, dt)

    def view(self, buf=None):
        buf = self.buf if buf is None else buf
        return buf[:self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.width]

    def outside(self, buf):
        m = np.ones(buf.size, bool)
        m[:self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.width] = False
        return buf[m]


def _ln_launch(lib, X, Y, fmt, w, b, rows, cols, drop=0, add=None, add2=None, ldadd=0, add_fmt=0, xsum=None, S=None, Y2=None):
    """Two launches, each on fresh device copies of x (a Rows), the output Y and the optional y2 (Rows) / separate xsum S (Rows);
    xsum = None / 'sep' / 'alias' (x itself).  Returns host (y, x, xsum, y2) of the first launch, asserting the second is bit-identical."""
    outs = []
    wd, bd = _dev(_f32(w)), _dev(_f32(b))
    for _ in range(2):
        xd, yd = _dev(X.buf), _dev(Y.buf)
        sd = xd if xsum == "alias" else (_dev(S.buf) if xsum == "sep" else None)
        y2d = _dev(Y2.buf) if Y2 is not None else None
        _chk(lib, lib.ec_op_layernorm_ex(_p(xd), X.ld, _p(yd), Y.ld, fmt, _p(wd), _p(bd), rows, cols, EPS, drop, _p(add), _p(add2),
                                          ldadd, add_fmt, _p(sd), _p(y2d), Y2.ld if Y2 is not None else 0, None))
        torch.cuda.synchronize()
        outs.append((_host(yd, Y.dt), _host(xd, np.float32), _host(sd, np.float32) if sd is not None else None,
                     _host(y2d, np.uint16) if y2d is not None else None))
    for a, c in zip(*outs):
        assert (a is None and c is None) or np.array_equal(a.view(np.uint8), c.view(np.uint8)), "second launch differs"
    return outs[0]


def _sent(dt):
    return np.uint16(SENT16) if dt == np.uint16 else np.array(SENT32, np.uint32).view(np.float32)


def _assert_sentinels(Y, out):
    raw = Y.outside(out).view(np.uint16 if Y.dt == np.uint16 else np.uint32)
    want = SENT16 if Y.dt == np.uint16 else SENT32
    assert np.all(raw == want), f"{int((raw != want).sum())} elements written outside the output"


def _check_out(fmt, got, ref, gate):
    """Output format rules against the fp64 reference and its fp32 gate (ln_gate)."""
    if fmt == 0:
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err <= gate), float((err / gate).max())
        return
    if fmt in (1, 2):
        p, emin = (8, -126) if fmt == 1 else (11, -14)
        y = (R.dec_bf16 if fmt == 1 else R.dec_f16)(got)
        rr = (R.rne_bf16 if fmt == 1 else R.rne_f16)(ref)
        assert np.isfinite(y).all()
        # y = RNE(v) for the kernel's fp32 v, |v - ref| <= gate: within half an ulp (of v's binade) + gate of ref, never 1 ulp off RNE(ref)
        assert np.all(np.abs(y - ref) <= 0.5 * R.ulp(np.abs(ref) + gate, p, emin) + gate)
        # where the fp32 gate is at most a quarter of the format's ulp, the kernel stores RNE(ref) or a neighbour, never an ulp off.
        # Elsewhere the fp32 error may span ulps of the format and the half-ulp + gate rule above is the contract: outputs near 0 where
        # w xhat and b cancel, and the offset rows, whose fp32 mean is off by up to ~1e-4 (ln_gate).
        # How often RNE(v) != RNE(ref): a rounding tie lies between v and ref with probability 2 |v - ref| / ulp for ref spread evenly over
        # its ulp, so the expected share is at most mean(2 gate / ulp).  For bf16 that is far below 0.1 %; for fp16 it is not - fp32
        # arithmetic at ~16 u of |w xhat| + |b| against fp16's half ulp of 2^-12 |y| leaves 0.1 - 0.5 % of the elements (measured) on
        # the other side of a tie, so the share allowed is that bound, and never less than 0.1 %.
        sel = gate <= 0.25 * R.ulp(rr, p, emin)
        assert sel.mean() > 0.5, float(sel.mean())
        u16 = R.ulp(rr[sel], p, emin)
        assert np.all(np.abs(y[sel] - rr[sel]) <= u16)
        allowed = max(1e-3, float(np.mean(2 * gate[sel] / u16)))
        assert (y[sel] != rr[sel]).mean() <= allowed, (float((y[sel] != rr[sel]).mean()), allowed)
        return
    n = ref.shape[-1]
    if fmt == 3:
        hi, lo = R.dec_split_bf16(got, n)
        # lo = bf16(v - hi): |v - hi| <= 2^-8 |v|, rounded to 8 bits: hi + lo is within 2^-16 |v| of v
        assert np.all(np.abs(hi + lo - ref) <= gate + 2.0 ** -16 * (np.abs(ref) + gate))
        assert np.all(np.abs(hi - ref) <= 2.0 ** -8 * (np.abs(ref) + gate) + gate)
        return
    hi, lo8, hi8 = R.dec_x2(got, n)
    assert np.isfinite(hi).all()
    assert np.all(np.abs(hi + lo8 - ref) <= gate + 2.0 ** -14 * (np.abs(ref) + gate) + 2.0 ** -28)
    assert np.all(np.abs(hi - ref) <= 2.0 ** -11 * (np.abs(ref) + gate) + gate + 2.0 ** -25)
    assert np.all(np.abs(hi8 - ref) <= 2.0 ** -3 * (np.abs(ref) + gate) + gate + 2.0 ** -17)


def _ywidth(fmt, cols):
    return 2 * cols if fmt in (3, 6) else cols


@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 6])
@pytest.mark.parametrize("cols", [132, 256, 384, 768, 1024])
@pytest.mark.parametrize("rows", [1, 3, 4099])
def test_ln_formats(lib, rows, cols, fmt):
    """Every output format of layernorm_kernel at the model's widths (132: the c < cols tails), x rows of stride cols + 12 with NaN
    slack, outputs of stride width + 8 with sentinel slack and sentinel rows after the last one."""
    x, w, b, kind = _ln_data(rows, cols)
    ref, gate = _ln_ref(x, w, b)
    X = Rows(rows, cols, cols + 12, np.float32, np.nan)
    X.view()[:] = x
    dt = np.float32 if fmt == 0 else np.uint16
    Y = Rows(rows, _ywidth(fmt, cols), _ywidth(fmt, cols) + 8, dt, _sent(dt))
    out = _ln_launch(lib, X, Y, fmt, w, b, rows, cols)[0]
    _assert_sentinels(Y, out)
    got = Y.view(out)
    if fmt == 0:
        gauss = kind == 0
        assert np.abs(got[gauss] - ref[gauss]).max() < 2e-5      # today's cap of test_gpu_ops.py test_layernorm holds as well
    _check_out(fmt, got, ref, gate)


@pytest.mark.parametrize("xsum", ["none", "sep", "alias"])
@pytest.mark.parametrize("nbr", [1, 2])
@pytest.mark.parametrize("out", ["f32", "h16"])
@pytest.mark.parametrize("afmt", [1, 2])
@pytest.mark.parametrize("cols", [132, 768])
def test_ln_fused_add(lib, cols, afmt, out, nbr, xsum):
    """Residual add of one or two pending 16-bit branches fused in front of the norm (bf16 / fp16 backbone): x' = (x + add) + add2,
    two fp32 additions in that order, written to xsum (a separate buffer, x itself, or nowhere) and normalised; fp32 output or the
    branch's own 16-bit format."""
    rows = 1027
    g = _rng("lnadd", cols, afmt, nbr)
    x = (g.standard_normal((rows, cols)) * 2.0).astype(np.float32)
    w = g.standard_normal(cols).astype(np.float32)
    b = g.standard_normal(cols).astype(np.float32)
    enc, rnd = (R.bf16_bits, R.rne_bf16) if afmt == 1 else (R.f16_bits, R.rne_f16)
    ld = cols + 8
    X = Rows(rows, cols, ld, np.float32, np.nan)
    X.view()[:] = x
    brs = []
    for i in range(nbr):
        A = Rows(rows, cols, ld, np.uint16, NAN16)
        A.view()[:] = enc(g.standard_normal((rows, cols)) * 0.5)
        brs.append(A)
    xs = x.copy()
    for A in brs:
        xs = xs + R.dec_bf16(A.view()).astype(np.float32) if afmt == 1 else xs + R.dec_f16(A.view()).astype(np.float32)
    ref, gate = _ln_ref(xs.astype(np.float64), w.astype(np.float64), b.astype(np.float64))
    S = Rows(rows, cols, ld, np.float32, _sent(np.float32))
    fmt = 0 if out == "f32" else afmt
    dt = np.float32 if fmt == 0 else np.uint16
    Y = Rows(rows, cols, cols + 4, dt, _sent(dt))
    a1 = _dev(brs[0].buf)
    a2 = _dev(brs[1].buf) if nbr == 2 else None
    res, xa, sa, _ = _ln_launch(lib, X, Y, fmt, w, b, rows, cols, add=a1, add2=a2, ldadd=ld, add_fmt=afmt if fmt == 0 else 0,
                                 xsum=None if xsum == "none" else xsum, S=S)
    _assert_sentinels(Y, res)
    _check_out(fmt, Y.view(res), ref, gate)
    if xsum == "none":
        assert np.array_equal(xa.view(np.uint32), X.buf.view(np.uint32)), "x changed without xsum"
        return
    Sv = Rows(rows, cols, ld, np.float32, 0)
    assert np.array_equal(Sv.view(sa).view(np.uint32), xs.view(np.uint32)), "xsum is not the fp32 sum (x + add) + add2"
    base = X.buf if xsum == "alias" else S.buf
    assert np.array_equal(Sv.outside(sa).view(np.uint32), Sv.outside(base).view(np.uint32)), "xsum written outside its rows"


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ln_drop_period(lib, fmt):
    """The backbone's final norm drops the cls row of every image: input row n T + t (t >= 1) -> output row n (T - 1) + t - 1;
    exactly n (T - 1) rows are written."""
    T, n, cols = 257, 3, 384
    x, w, b, _ = _ln_data(n * T, cols)
    ref, gate = _ln_ref(x, w, b)
    keep = np.arange(n * T) % T != 0
    X = Rows(n * T, cols, cols + 4, np.float32, np.nan)
    X.view()[:] = x
    dt = np.float32 if fmt == 0 else np.uint16
    Y = Rows(n * (T - 1), cols, cols, dt, _sent(dt), tail=8)
    out = _ln_launch(lib, X, Y, fmt, w, b, n * T, cols, drop=T)[0]
    _assert_sentinels(Y, out)
    _check_out(fmt, Y.view(out), ref[keep], gate[keep])


def test_ln_y2_side_copy(lib):
    """The head's image-memory update: fp32 output plus an fp16 copy y2 (stride ldy2) that is exactly fp16(y) of the stored fp32 y."""
    rows, cols = 1000, 256
    x, w, b, _ = _ln_data(rows, cols)
    ref, gate = _ln_ref(x, w, b)
    X = Rows(rows, cols, cols + 4, np.float32, np.nan)
    X.view()[:] = x
    Y = Rows(rows, cols, cols, np.float32, _sent(np.float32))
    Y2 = Rows(rows, cols, cols + 8, np.uint16, SENT16)
    out, _, _, y2 = _ln_launch(lib, X, Y, 0, w, b, rows, cols, Y2=Y2)
    _assert_sentinels(Y, out)
    _check_out(0, Y.view(out), ref, gate)
    _assert_sentinels(Y2, y2)
    assert np.array_equal(Y2.view(y2), R.f16_bits(Y.view(out).astype(np.float64)))


@pytest.mark.parametrize("where", ["f16", "x2", "y2"])
def test_ln_fp16_saturation_and_nan(lib, where):
    """fp16 outputs (OUT 2, the fp16 plane of OUT 6, y2): values past +-65504 saturate to +-65504, not inf; a NaN in one input row
    makes that row NaN and leaves every other row bit for bit as without it (test_linear_h16_fp16_nan_in_nan_out's contract)."""
    rows, cols = 64, 256
    x, w, b, _ = _ln_data(rows, cols)
    w = w.copy()
    w[5] = 3e5                                    # |y| ~ 3e5 |xhat| in column 5: past 65504 in most rows
    ref, _ = _ln_ref(x, w, b)
    fmt = {"f16": 2, "x2": 6, "y2": 0}[where]
    res = []
    for poison in (False, True):
        X = Rows(rows, cols, cols, np.float32, 0)
        X.view()[:] = x
        if poison:
            X.view()[7, 3] = np.nan
        dt = np.float32 if fmt == 0 else np.uint16
        Y = Rows(rows, _ywidth(fmt, cols), _ywidth(fmt, cols), dt, _sent(dt))
        Y2 = Rows(rows, cols, cols, np.uint16, SENT16)
        out, _, _, y2 = _ln_launch(lib, X, Y, fmt, w, b, rows, cols, Y2=Y2 if where == "y2" else None)
        res.append(Y2.view(y2) if where == "y2" else Y.view(out))
    clean, dirty = res
    h = R.dec_f16(clean[:, :cols])
    big = np.abs(ref) > 65504.0
    assert big.sum() > rows // 4 and not big[:, np.arange(cols) != 5].any()
    assert np.isfinite(h).all()
    assert np.all(h[big] == np.sign(ref[big]) * 65504.0)
    hd = R.dec_f16(dirty[:, :cols])
    assert np.isnan(hd[7]).all(), "the NaN row is not NaN"
    others = np.arange(rows) != 7
    assert np.array_equal(dirty[others], clean[others]), "a NaN row changed other rows"
