"""Float64 reference of the codec, ONE LAUNCH AT A TIME (host only; test infrastructure).

Every launch of a one-shot decode / encode (the launch trace of include/fishtts_hip_test.h) is one `Stage` here:
a plan (`plan_decode`, `plan_encode`) lists them in launch order with the logical buffers each reads and writes,
restating the data flow of oracle/codec.py (CodecOracle.quantizer_decode / decoder / encoder / quantizer_encode), and
`eval_stage` evaluates one of them from the values its inputs held.  Three uses:

  * mode "free":    float64 throughout, unrounded f32 weights, own outputs as inputs: the plan chained over a whole
                    decode / encode must reproduce the oracle (tests/test_codec_stage_ref_host.py pins this);
  * mode "check":   teacher forcing: the RECORDED inputs of a launch (exact bf16 / f32 values), the weights as the
                    device holds them (bf16-rounded MFMA operands; f32 bias, alpha, gamma, depthwise and norm weights)
                    -> float64 `ref` per written buffer, plus `err`, a bound on |value before the store - ref| derived
                    below.  `check_stage` then demands, of every checked element,
                        |got - ref| <= half a ulp of the stored format at max(|got|, |ref|) + err;
  * mode "emulate": the same operation in float32 (contractions summed per 32-wide k block, the blocks in order) with
                    bf16 / f32 stores: an honest stand-in for the device, from which the host tests build synthetic
                    traces, with and without injected bugs.

Error model (u = 2^-24, the float32 unit round-off; every float32 operation returns its exact result times (1 + d),
|d| <= u):

  contraction of n = taps x K products.  bf16 x bf16 is exact in float32, so the only error is the accumulation's.  In
      any order it is below n 2^-23 S, S = sum |x| |w| (the ceiling; it also covers a truncating adder), but that is
      tens of bf16 steps wide at n ~ 10^4.  The working bound is measured on the reference alone: the same sums in
      float32 in three orders (k ascending as one chain with the taps outermost; one partial sum per 32-wide k block,
      blocks in order; pairwise) on a seeded subset of the checked elements (<= R_ORDER_ROWS rows x R_ORDER_COLS
      columns: a maximum over fewer elements is smaller, so the subset only tightens the bound), r_stage = the largest
      |f32 - f64| / S, and E = min(4 r_stage, n 2^-23) S.
  epilogue, tracked op by op: v = acc + bias: err = E + u |v|.  GELU (Lipschitz <= 1.13; erff to 2^-20 absolute on
      |erf| <= 1): err = 1.13 err + |v| / 2 (2^-20 + 2 u) + 2 u |g|.  SwiGLU o = silu(gate) up, silu Lipschitz <= 1.1,
      expf to 2^-20 relative: err = |up| (1.1 e_gate + (2^-20 + 3 u) |silu|) + |silu| e_up + 1.1 e_gate e_up + u |o|.
      Column scale: err = |gamma| err + u |v|.  Residual add: err = err + u |v|.  Snake y = v + sin^2(a v) / a
      (Lipschitz <= 2; __sinf to 1e-6 absolute as snake_f's comment claims, its argument a v rounded once):
      err_y = 2 err + 2 |sin| / a (1e-6 + u |a v|) + 4 u (|v| + sin^2 / a).
  RMSNorm over D: the sum of squares has non-negative terms, D / 256 per thread, 6 + 3 tree steps, / D, + eps:
      relative error <= (D / 256 + 11) u; 1 / sqrt halves it and adds 2 u, two products add 2 u:
      err = (D / 512 + 10) u |ref|.
  RoPE: two products and one sum: err = 2 u (|x0 c| + |x1 s|); the v third is copied.
  attention over nk keys: a score is an hd-term chain times the scale: ds = (hd + 2) u scale sum |q| |k|; the
      exponent s - max adds u |s - max|; an absolute error D in the exponent is a relative e^D - 1 in the weight, expf
      adds 2^-20; numerator and denominator both carry it, the sum adds (nk / 64 + 8) u, the P V chain (nk + 2) u:
      err = (2 (D + 2^-20) + (nk + nk / 64 + 12) u) sum softmax_j |v_j|,  D = max_j (ds_j + u |s_j - max|).
  depthwise k = 7 + LayerNorm over C: a = bias + 7 products: ea = 8 u (|b| + sum |w| |x|); mean: dm = mean(ea) +
      (C / 256 + 10) u mean |a|; d = a - mean: dd = ea + dm + u |d|; var: dv = 2 mean(|d| dd) + (C / 256 + 10) u var;
      1 / sqrt(var + eps): relative ri = dv / (2 (var + eps)) + 3 u; y = d inv lw + lb:
      err = |lw| inv (dd + |d| ri) + 3 u (|d inv lw| + |lb|).
  final k = 7 convolution + tanh: f32 weights, each lane a chain of 7 x 8 fused multiply-adds, a 4-step tree, the bias:
      err = (7 max(8, ceil(C / 16)) + 6) u (S + |b|); tanh is 1-Lipschitz, tanhf to 2^-20 relative:
      err = err + (2^-20 + u) |tanh|.
  first encoder convolution (1 channel, k = 7, f32): err = 8 u (|b| + sum |w| |x|), then the stores / Snake as above.
  RVQ gather: each table entry is codebook_dim products and the bias in f32 at load time, then 1 + n_codebooks entries
      are summed: err = sum_i (cd + 1) u (sum |w| |cb| + |b|)_i + (n_codebooks + 1) u sum_i |table_i|.

The quantiser search (rvq_encode_kernel; `rvq_search_check`) returns integers, so it is judged per DECISION, not per
element: one decision per (frame, codebook).  The reference restates CodecOracle._vq / quantizer_encode in float64,
teacher-forced on the device's picks: at codebook q the residual is the recorded zq minus the float64 table rows of the
device's picks 0 .. q-1, its score of row i is s_i = -(|en|^2 - 2 en . c_i + |c_i|^2) with en = e / |e|, e = in_proj
(residual), c_i the L2-normalised codebook row, and the device's pick must have s_pick >= max_i s_i - b.  Codebook rows
that are bit-identical in float32 have identical device scores (cbn, cn2 and the dot chain are functions of the row
alone), and the kernel keeps the lowest index on equal scores within a thread, across lanes and across waves: a pick
that is not the lowest index of its group of bit-identical rows is a fault, with no tolerance.
    The device takes the argmax of s~_i = s_i + c + eta_i, c common to all rows of the decision (its |en|^2 is not
exactly 1), |eta_i| <= eps; then s_pick >= s_best - 2 eps, so b = 2 eps, and eps collects, with cd = codebook_dim and
|en| = |c_i| = 1 (so sum_k |en_k| |c_ik| <= 1, |2 en . c_i| <= 2, |s_i| <= 4):
  projection: products of f32 operands are exact in f64, D / 256 fused terms per thread, a 6-step tree, three sums and
      the bias in f64, then ONE rounding to f32: de_k = u |e_k| + (D / 256 + 12) 2^-53 (sum |W| |res| + |b|)_k
      + sum_d |W_kd| dres_d, dres the distance of the device's f32 residual from the reference's (below).  A
      perturbation de of e moves en by at most 2 |de| / |e| and a score by twice that: 4 |de|_2 / |e|_2.
  norm and reciprocal: nn a cd-term chain of non-negative terms (cd u relative), the square root halves it and adds u,
      the reciprocal adds u (2 u if approximated), the product en_k = e_k inv u: a common relative error (cd / 2 + 4) u
      of en that scales 2 en . c_i (row-dependent): 2 (cd / 2 + 4) u; the product's own rounding, per component: 2 u.
  normalised codebook at load (normalize_codebook_kernel): the same chain per row, c~_i = c_i (1 + rho),
      |rho| <= (cd / 2 + 4) u, and cn2 a cd-term chain on the stored c~: -2 en . c~_i + |c~_i|^2 is off by
      2 |rho| + 2 |rho| + cd u = (3 cd + 16) u.
  the cd-term fma chain of the dot: cd u sum |en_k| |c_ik| <= cd u, doubled (2.0f * dot is exact): 2 cd u.
  three-term score: (l2 - 2 dot) rounds at |.| <= 3, the sum with cn2 at |.| <= 4: 7 u.
      Together (cd + 8) u + 2 u + (3 cd + 16) u + 2 cd u + 7 u = (6 cd + 33) u: 4.8e-6 at cd = 8.
  residual: the table built in f32 at load (the gather stage's term, (cd + 1) u (sum |w| |cb| + |b|) per entry) and one
      f32 subtraction per codebook: dres_d += (cd + 1) u (sum |w| |cb| + |b|)_d + u |res_d| after every pick.
  eps = (6 cd + 33) u + 4 |de|_2 / |e|_2.
    At the first codebook dres = 0 and b is about 1e-5.  From the second on, sum_d |W_kd| dres_d is a sum of D absolute
values whose signs a worst case may not let cancel: it reaches 2e-3 at D = 1024 (tests/test_codec_stage_ref_host.py
prints it beside b; the honest float32 search there never leaves the float64 argmax), more than the 5e-5 the search
was already held to on the oracle's latents (the accumulation error of a 1024-term f32 sum on scores of O(1):
tests/test_codec_gpu.py).  b is therefore the SMALLER of the two,
b = min(2 eps, 5e-5): nowhere wider than the bound the search already had, tighter where the derivation is.  A pick
other than the float64 argmax must lie inside b, and at most 1 % of a case's decisions may be such picks
(RVQ_NON_ARGMAX_CAP; the float32 emulation has none in 1290 decisions at the real widths).

Carried context (the streamed decode: ft_codec_stream_decode, one chunk of ft_codec_stream_decode_many).  `plan_stream`
lists the launches of ONE chunk of T frames at rope position t0 with nh = min(t0, window - 1) carried K/V rows: the
launches of plan_decode on the chunk's codes, plus the carrying launches, which are stages of their own:
  "<stage>.roll" (kind roll) in front of every stage with a halo H: "front" = the carry the previous chunk left for that
      stage (H x C; zeros before the first chunk), "carry" = the last H rows of (front ++ the chunk's T m input rows);
  "post.<l>.kvin" (kind kvin; only when nh > 0): "front" = the last nh rows of the layer's K/V carry ((window-1) x 2 HD);
  "post.<l>.kvout" (kind kvout): "carry" = the last min(window - 1, nh + T) rows of (front ++ the chunk's rotated K / V),
      placed at the END of the (window-1)-row carry.  The rows in front of them are not written: they hold zeros, because
      the number of rows kept never shrinks from chunk to chunk, so no earlier chunk wrote there in either copy.
The arithmetic stages then read "rows before 0" from the recorded front instead of the causal zero padding (gather's
`stale=` path: tap GEMMs, dwln, final); RoPE takes rows t0 + i of the table; attention puts the nh front rows before the
chunk's keys, query i seeing keys [max(0, nh + i - window + 1), nh + i] of the nh + T.  Their error bounds are the ones
above, unchanged: the carried rows are operands like any other.  The carrying stages are pure copies: they are
restated on the recorded bit patterns and accepted bit for bit only (bound 0).  Carries live in env under "carry:..."
keys from chunk to chunk (`carries`); a chunk traced after untraced chunks is judged on the front rows it recorded
(`seed_unlinked`).  A batched call is the same plan per chunk on the chunk's rows of the dense records.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from oracle import codec as OC

U = 2.0 ** -24
LIB = 2.0 ** -20            # erff / expf / tanhf: 16 f32 ulp, 2048 times below the bf16 step
SIN_ABS = 1e-6              # __sinf, as snake_f's comment in csrc/gemm_kernels.h claims
MARGIN = 4.0                # E = MARGIN * r_stage * S
R_ORDER_ROWS, R_ORDER_COLS = 256, 48
F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------- number formats
def bf16_bits(x: torch.Tensor) -> np.ndarray:
    """float -> bf16 bit patterns (round to nearest even, as f32_to_bf16_bits)."""
    return x.to(F32).to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def h16_bits(x: torch.Tensor, fmt: str = "bf16") -> np.ndarray:
    """float -> bit patterns of a 16-bit format, "bf16" or "fp16" (round to nearest even, overflow to infinity, fp16
    subnormals included: the conversions of common.h)."""
    if fmt == "bf16":
        return bf16_bits(x)
    return x.to(F32).to(torch.float16).contiguous().view(torch.int16).numpy().view(np.uint16)


def from_raw(a, fmt: str = "bf16") -> torch.Tensor:
    """A recorded buffer (uint16 bit patterns of `fmt`, or float32) or a tensor -> a tensor of its exact values."""
    if isinstance(a, torch.Tensor):
        return a
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16 if fmt == "bf16" else torch.float16).to(F32)
    return torch.from_numpy(a)


def half_ulp(mag: torch.Tensor, f32: bool, fmt: str = "bf16") -> torch.Tensor:
    """Half a unit in the last place at |mag|: 2^(e-8) (bf16) / 2^(e-24) (f32) / 2^(e-11) (fp16) for a magnitude in
    [2^e, 2^(e+1)); below the smallest normal number (2^-126; 2^-14 in fp16) the step stays that of the lowest binade
    (fp16: 2^-24, so half of it 2^-25)."""
    fp16 = fmt == "fp16" and not f32
    _, ex = torch.frexp(mag.to(F64).abs().clamp_min(2.0 ** (-14 if fp16 else -126)))       # mag = f * 2^ex, f in [0.5, 1): e = ex - 1
    return torch.ldexp(torch.ones_like(mag, dtype=F64), ex - 1 - (24 if f32 else 11 if fp16 else 8))


# ------------------------------------------------------------------------------------------------------- the plan
@dataclass
class Stage:
    name: str
    kind: str                     # gemm | rvq | rmsnorm | rope | attn | dwln | final | enc_in | snake | tof32 | roll | kvin | kvout
    rows: int
    cols: int
    src: Dict[str, str] = field(default_factory=dict)     # role ("x", "resid") -> logical buffer
    dst: Dict[str, str] = field(default_factory=dict)     # "bf" | "act" | "f32" -> logical buffer
    p: dict = field(default_factory=dict)

    @property
    def stat_kind(self) -> str:
        return "gemm." + self.p["pack"][0] if self.kind == "gemm" else self.kind

    @property
    def halo(self) -> int:
        if self.kind in CARRY_KINDS:
            return self.rows
        if self.kind == "gemm":
            return max(0, -min(self.p["offs"]))
        return 6 if self.kind in ("dwln", "final", "enc_in") else 0


def _gemm(name, rows, x, K, N, pack, offs, dst, bias=None, act="none", gamma=None, resid=None, alpha=None, n_mod=None):
    cols = N // 2 if act == "swiglu" else N
    src = {"x": x}
    if resid:
        src["resid"] = resid[0]
    return Stage(name, "gemm", rows, cols, src, dst,
                 dict(K=K, N=N, pack=pack, offs=offs, bias=bias, act=act, gamma=gamma, alpha=alpha,
                      resid_f32=bool(resid and resid[1] == "f32"), n_mod=n_mod or N))


def _tf(out: List[Stage], pfx, wp, n_layer, T, D, H, hd, ffn, window, base, eps, final_dst):
    """One window-limited transformer (CodecOracle._window_transformer / _tf_block) over the f32 stream "x"."""
    tab = OC.rope_table(T, hd, base).to(F32)            # bf16-rounded cos / sin, as both the oracle and the engine build it
    HD = H * hd
    for l in range(n_layer):
        p = f"{wp}.layers.{l}"
        out.append(Stage(f"{pfx}{l}.norm1", "rmsnorm", T, D, {"x": "x"}, {"bf": "xn"}, dict(w=f"{p}.attention_norm.weight", eps=eps)))
        out.append(_gemm(f"{pfx}{l}.qkv", T, "xn", D, 3 * HD, ("linear", f"{p}.attention.wqkv.weight"), [0], {"bf": "qkv"}))
        out.append(Stage(f"{pfx}{l}.rope", "rope", T, 3 * HD, {"x": "qkv"}, {"bf": "qkv"}, dict(H=H, hd=hd, tab=tab)))
        out.append(Stage(f"{pfx}{l}.attn", "attn", T, HD, {"x": "qkv"}, {"bf": "y"}, dict(H=H, hd=hd, window=window)))
        out.append(_gemm(f"{pfx}{l}.wo", T, "y", HD, D, ("linear", f"{p}.attention.wo.weight"), [0], {"f32": "x"},
                         gamma=f"{p}.attention_layer_scale.gamma", resid=("x", "f32")))
        out.append(Stage(f"{pfx}{l}.norm2", "rmsnorm", T, D, {"x": "x"}, {"bf": "xn"}, dict(w=f"{p}.ffn_norm.weight", eps=eps)))
        out.append(_gemm(f"{pfx}{l}.w13", T, "xn", D, 2 * ffn, ("w13", f"{p}.feed_forward.w1.weight", f"{p}.feed_forward.w3.weight"),
                         [0], {"bf": "g"}, act="swiglu"))
        out.append(_gemm(f"{pfx}{l}.w2", T, "g", ffn, D, ("linear", f"{p}.feed_forward.w2.weight"), [0], {"f32": "x"},
                         gamma=f"{p}.ffn_layer_scale.gamma", resid=("x", "f32")))
    out.append(Stage(f"{pfx}norm", "rmsnorm", T, D, {"x": "x"}, final_dst, dict(w=f"{wp}.norm.weight", eps=eps)))


def _convnext(out, name, wp, rows, D, u, n, h, z_dst):
    out.append(Stage(f"{name}.dwln", "dwln", rows, D, {"x": u}, {"bf": n},
                     dict(w=f"{wp}.dwconv.conv.weight", b=f"{wp}.dwconv.conv.bias", lw=f"{wp}.norm.weight", lb=f"{wp}.norm.bias")))
    out.append(_gemm(f"{name}.pw1", rows, n, D, 4 * D, ("linear", f"{wp}.pwconv1.weight"), [0], {"bf": h},
                     bias=f"{wp}.pwconv1.bias", act="gelu"))
    out.append(_gemm(f"{name}.pw2", rows, h, 4 * D, D, ("linear", f"{wp}.pwconv2.weight"), [0], z_dst,
                     bias=f"{wp}.pwconv2.bias", gamma=f"{wp}.gamma", resid=(u, "bf")))


def plan_decode(c: OC.CodecShape, codes) -> List[Stage]:
    """The launches of one decode of codes (1 + n_codebooks, T), in order (CodecOracle.decode restated per launch)."""
    codes = torch.as_tensor(np.asarray(codes)).long()
    T, D = codes.shape[1], c.latent_dim
    out = [Stage("rvq", "rvq", T, D, {}, {"f32": "x"}, dict(codes=codes))]
    _tf(out, "post.", "quantizer.post_module", c.n_tf_layer, T, D, c.tf_n_head, c.tf_head_dim, c.tf_ffn, c.tf_window,
        c.tf_rope_base, c.tf_norm_eps, {"bf": "z"})
    Tc = T
    for j, f in enumerate(c.upsample):
        wp = f"quantizer.upsample.{j}"
        out.append(_gemm(f"up.{j}.ct", Tc, "z", D, f * D, ("convT", f"{wp}.0.conv.weight", f), [0],
                         {"bf": "u"}, bias=f"{wp}.0.conv.bias", n_mod=D))
        Tc *= f
        _convnext(out, f"up.{j}", f"{wp}.1", Tc, D, "u", "n", "h", {"bf": "z"})
    ch = c.decoder_dim
    out.append(_gemm("dec.in", Tc, "z", D, ch, ("conv", "decoder.model.0.conv.weight", 1), [k - 6 for k in range(7)], {"act": "a"},
                     bias="decoder.model.0.conv.bias", alpha="decoder.model.1.block.0.alpha"))
    nb = len(c.rates)
    for bi, r in enumerate(c.rates):
        cin, cout = ch >> bi, ch >> (bi + 1)
        p = f"decoder.model.{bi + 1}.block"
        out.append(_gemm(f"dec.{bi}.ct", Tc, "a", cin, r * cout, ("convT", f"{p}.1.conv.weight", r), [0, -1], {"bf": "r", "act": "a2"},
                         bias=f"{p}.1.conv.bias", alpha=f"{p}.2.block.0.alpha", n_mod=cout))
        Tc *= r
        for ui, d in enumerate((1, 3, 9)):
            q = f"{p}.{ui + 2}.block"
            out.append(_gemm(f"dec.{bi}.u{ui}.c7", Tc, "a2", cout, cout, ("conv", f"{q}.1.conv.weight", d),
                             [(k - 6) * d for k in range(7)], {"act": "hs"}, bias=f"{q}.1.conv.bias", alpha=f"{q}.2.alpha"))
            nxt = (f"{p}.{ui + 3}.block.0.alpha" if ui < 2 else
                   f"decoder.model.{bi + 2}.block.0.alpha" if bi + 1 < nb else f"decoder.model.{nb + 1}.alpha")
            dst = {"bf": "r", "act": "a2"} if ui < 2 else {"act": "a"}
            out.append(_gemm(f"dec.{bi}.u{ui}.c1", Tc, "hs", cout, cout, ("conv", f"{q}.3.conv.weight", 1), [0], dst,
                             bias=f"{q}.3.conv.bias", resid=("r", "bf"), alpha=nxt))
    out.append(Stage("final", "final", Tc, 1, {"x": "a"}, {"f32": "audio"},
                     dict(w=f"decoder.model.{nb + 2}.conv.weight", b=f"decoder.model.{nb + 2}.conv.bias", C=ch >> nb)))
    return out


def plan_encode(c: OC.CodecShape, audio) -> List[Stage]:
    """The launches of one encode of mono audio up to the pre-quantiser latents ("zq"), in order (CodecOracle.encode)."""
    audio = torch.as_tensor(np.asarray(audio, dtype=np.float32)).reshape(-1)
    fl = c.enc_frame_len
    T = int(math.ceil(audio.numel() / fl) * fl)
    audio = torch.nn.functional.pad(audio, (0, T - audio.numel()))
    D, d = c.latent_dim, c.encoder_dim
    r_, o_ = "r", "o"
    out = [Stage("enc.in", "enc_in", T, d, {}, {"bf": r_, "act": "a"},
                 dict(audio=audio, w="encoder.block.0.conv.weight", b="encoder.block.0.conv.bias",
                      alpha="encoder.block.1.block.0.block.0.alpha"))]
    nb = len(c.encoder_rates)
    for bi, (s, nt) in enumerate(zip(c.encoder_rates, c.encoder_tf_layers)):
        p = f"encoder.block.{bi + 1}.block"
        for ui, dil in enumerate((1, 3, 9)):
            q = f"{p}.{ui}.block"
            out.append(_gemm(f"enc.{bi}.u{ui}.c7", T, "a", d, d, ("conv", f"{q}.1.conv.weight", dil), [(k - 6) * dil for k in range(7)],
                             {"act": "hs"}, bias=f"{q}.1.conv.bias", alpha=f"{q}.2.alpha"))
            nxt = f"{p}.{ui + 1}.block.0.alpha" if ui < 2 else f"{p}.3.alpha"
            dst = {"bf": r_, "act": "a"} if ui < 2 else {"act": "a"}
            out.append(_gemm(f"enc.{bi}.u{ui}.c1", T, "hs", d, d, ("conv", f"{q}.3.conv.weight", 1), [0], dst,
                             bias=f"{q}.3.conv.bias", resid=(r_, "bf"), alpha=nxt))
        T //= s
        out.append(_gemm(f"enc.{bi}.sc", T, "a", s * d, 2 * d, ("strided", f"{p}.4.conv.weight", s), [-1, 0],
                         {"f32": "x"} if nt else {"bf": o_}, bias=f"{p}.4.conv.bias"))
        d *= 2
        if nt:
            _tf(out, f"enc.{bi}.tf.", f"{p}.5", nt, T, d, d // 64, 64, 3 * d, c.enc_tf_window, c.tf_rope_base, c.tf_norm_eps, {"bf": o_})
        nxt = f"encoder.block.{bi + 2}.block.0.block.0.alpha" if bi + 1 < nb else f"encoder.block.{nb + 1}.alpha"
        out.append(Stage(f"enc.{bi}.snake", "snake", T, d, {"x": o_}, {"act": "a"}, dict(alpha=nxt)))
        r_, o_ = o_, r_
    wp = f"encoder.block.{nb + 2}.conv"
    out.append(_gemm("enc.out", T, "a", d, D, ("conv", f"{wp}.weight", 1), [-2, -1, 0], {"bf": "ez"}, bias=f"{wp}.bias"))
    for j, f in enumerate(c.upsample):
        wp = f"quantizer.downsample.{j}"
        T //= f
        out.append(_gemm(f"down.{j}.sc", T, "ez", f * D, D, ("strided", f"{wp}.0.conv.weight", f), [0], {"bf": "u"},
                         bias=f"{wp}.0.conv.bias"))
        last = j + 1 == len(c.upsample)
        _convnext(out, f"down.{j}", f"{wp}.1", T, D, "u", "n", "h", {"bf": "ez", "f32": "x"} if last else {"bf": "ez"})
    if not c.upsample:
        out.append(Stage("down.f32", "tof32", T, D, {"x": "ez"}, {"f32": "x"}))
    _tf(out, "pre.", "quantizer.pre_module", c.n_tf_layer, T, D, c.tf_n_head, c.tf_head_dim, c.tf_ffn, c.tf_window,
        c.tf_rope_base, c.tf_norm_eps, {"f32": "zq"})
    return out


CARRY_KINDS = ("roll", "kvin", "kvout")


def plan_stream(c: OC.CodecShape, codes_chunk, t0: int, nh: int) -> List[Stage]:
    """The launches of one chunk of a streamed decode, carrying launches included (see the module docstring): codes_chunk
    (1 + n_codebooks, T) are the chunk's codes, t0 the frames decoded before it, nh the carried K/V rows."""
    codes_chunk = torch.as_tensor(np.asarray(codes_chunk)).long()
    T, W1, HD = codes_chunk.shape[1], c.tf_window - 1, c.tf_n_head * c.tf_head_dim
    assert 0 <= nh == min(t0, W1), (t0, nh, W1)
    tab = OC.rope_table(t0 + T, c.tf_head_dim, c.tf_rope_base).to(F32)
    out: List[Stage] = []
    for st in plan_decode(c, codes_chunk):
        if st.kind == "rope":
            out.append(Stage(st.name, st.kind, st.rows, st.cols, dict(st.src), dict(st.dst), {**st.p, "tab": tab, "t0": t0}))
            pfx = st.name[:-len("rope")]
            if nh > 0:
                out.append(Stage(pfx + "kvin", "kvin", nh, 2 * HD, {"prev": f"carry:{pfx}kv"}, {"front": pfx + "kv.front"}, dict(W1=W1)))
            if W1 > 0:
                src = {"x": "qkv", **({"front": pfx + "kv.front"} if nh > 0 else {})}
                out.append(Stage(pfx + "kvout", "kvout", W1, 2 * HD, src, {"carry": f"carry:{pfx}kv"}, dict(HD=HD)))
        elif st.kind == "attn":
            src = {**st.src, **({"kv": st.name[:-len("attn")] + "kv.front"} if nh > 0 else {})}
            out.append(Stage(st.name, st.kind, st.rows, st.cols, src, dict(st.dst), {**st.p, "nh": nh}))
        elif st.halo > 0:
            C_in = st.p["K"] if st.kind == "gemm" else st.p["C"] if st.kind == "final" else st.cols
            out.append(Stage(st.name + ".roll", "roll", st.halo, C_in, {"x": st.src["x"], "prev": f"carry:{st.name}"},
                             {"front": st.name + ".front", "carry": f"carry:{st.name}"}))
            out.append(Stage(st.name, st.kind, st.rows, st.cols, {**st.src, "halo": st.name + ".front"}, dict(st.dst), dict(st.p)))
        else:
            out.append(st)
    return out


def carries(env: dict) -> dict:
    """What a chunk hands to the next one: the "carry:..." entries of its environment."""
    return {k: v for k, v in env.items() if k.startswith("carry:")}


def seed_unlinked(plan: List[Stage], outs: List[Dict[str, np.ndarray]]) -> dict:
    """The carries a chunk whose predecessor was not traced is judged on: those that make its own recorded front rows."""
    env = {}
    for st, o in zip(plan, outs):
        if st.kind == "roll":
            env[st.src["prev"]] = o["front"]
        elif st.kind == "kvin":
            full = np.zeros((st.p["W1"], st.cols), dtype=np.uint16)
            full[st.p["W1"] - st.rows:] = np.asarray(o["front"]).reshape(st.rows, st.cols)
            env[st.src["prev"]] = full
    return env


def producers(plan: List[Stage]) -> List[List[int]]:
    """For every stage, the indices of the launches whose recorded outputs it reads (the last writer of each source;
    a carry of an earlier chunk has none)."""
    last: Dict[str, int] = {}
    out = []
    for i, st in enumerate(plan):
        out.append(sorted({last[b] for b in st.src.values() if b in last}))
        for b in st.dst.values():
            last[b] = i
    return out


# ------------------------------------------------------------------------------------------------------ row subsets
def select_rows(M: int, halo: int, bm: int, seed: int = 0) -> torch.Tensor:
    """Rows to check of a stage of M rows whose launch works in row tiles of bm: all of them below 4096; else the first
    halo + 8, the last two row tiles (the ragged one), four rows on either side of (at least) eight interior tile
    boundaries, and 1024 further rows drawn with a fixed seed."""
    if M < 4096:
        return torch.arange(M)
    g = torch.Generator().manual_seed(1000003 * seed + M)
    pick = [torch.arange(min(M, halo + 8)), torch.arange(max(0, ((M - 1) // bm - 1) * bm), M)]
    nb = (M - 1) // bm                      # interior boundaries at bm, 2 bm, ..., nb bm
    bnd = torch.unique(torch.cat([torch.tensor([1, nb]), 1 + torch.randperm(nb, generator=g)[:10]]))
    for b in bnd.tolist():
        pick.append(torch.arange(max(0, b * bm - 4), min(M, b * bm + 4)))
    pick.append(torch.randperm(M, generator=g)[:1024])
    return torch.unique(torch.cat(pick))


# ------------------------------------------------------------------------------------------------------ evaluation
class Weights:
    """The folded f32 tensors; `dev=True` gives MFMA operands as the device holds them (rounded to bf16)."""

    def __init__(self, w: Dict[str, torch.Tensor], dev: bool):
        self.w, self.dev = w, dev

    def f(self, name) -> torch.Tensor:
        return self.w[name].to(F32).to(F64)

    def mm(self, name) -> torch.Tensor:
        t = self.w[name].to(F32)
        return (t.to(torch.bfloat16).to(F32) if self.dev else t).to(F64)


def pack(st: Stage, W: Weights) -> torch.Tensor:
    """[taps * K, N] float64: the contraction of this launch as one matrix, tap-major (restated from causal_conv,
    causal_convT, causal_conv_strided and F.linear in oracle/codec.py)."""
    kind, name = st.p["pack"][0], st.p["pack"][1]
    if kind == "w13":                                                  # columns: all gates, then all ups
        return torch.cat([W.mm(name).t(), W.mm(st.p["pack"][2]).t()], dim=1).contiguous()
    w = W.mm(name)
    if kind == "linear":
        return w.t().contiguous()
    if kind == "conv":                                                 # [Cout][Cin][k]: tap kk reads row t + (kk - (k-1)) d
        return torch.cat([w[:, :, kk].t() for kk in range(w.shape[2])], dim=0).contiguous()
    s = st.p["pack"][2]
    if kind == "convT":                                                # [Cin][Cout][k]: y[t s + r] = sum_j x[t - j] w[:, :, r + j s]
        return torch.cat([w[:, :, j * s:(j + 1) * s].permute(0, 2, 1).reshape(w.shape[0], -1) for j in range(w.shape[2] // s)], dim=0)
    if kind == "strided":                                              # [Cout][Cin][k]: y[t] = sum_kk w[:, :, kk] x[t s + kk - (k - s)]
        return torch.cat([w[:, :, a * s:(a + 1) * s].permute(2, 1, 0).reshape(-1, w.shape[0]) for a in range(w.shape[2] // s)], dim=0)
    raise ValueError(kind)


def gather(buf, C: int, rows: torch.Tensor, offs, stale=None) -> torch.Tensor:
    """[len(rows), len(offs) * C]: for every tap the row t + off of the [*, C] view of buf; rows before 0 are the causal
    zero padding (or `stale`, [halo, C], the rows an emulated bug reads there instead)."""
    raw = buf if isinstance(buf, torch.Tensor) else np.asarray(buf)
    v = raw.reshape(-1, C)
    parts = []
    for off in offs:
        idx = rows + off
        ok = idx >= 0
        if isinstance(v, torch.Tensor):
            x = v[idx.clamp_min(0)]
        else:
            x = from_raw(v[idx.clamp_min(0).numpy()])
        x = x.clone()
        if stale is not None:
            x[~ok] = stale.to(x.dtype)[(idx[~ok] + stale.shape[0])]
        else:
            x[~ok] = 0
        parts.append(x)
    return torch.cat(parts, dim=1)


def whole(buf, C: int) -> torch.Tensor:
    return from_raw(buf).reshape(-1, C)


def f32_orders(X: torch.Tensor, Wm: torch.Tensor) -> List[torch.Tensor]:
    """X [R, n] @ Wm [n, C] in float32 in three orders (operands are exact in float32)."""
    X, Wm = X.to(F32), Wm.to(F32)
    R, n = X.shape
    Cc = Wm.shape[1]
    Xt = X.t().contiguous()
    if R * n * Cc <= 1 << 21:     # few rows (a short streamed chunk): the same chain as one sequential float32 scan over k
        chain = torch.from_numpy(np.add.accumulate((X[:, :, None] * Wm[None]).numpy(), axis=1, dtype=np.float32)[:, -1].copy())
    else:
        chain = torch.zeros(R, Cc, dtype=F32)
        for t in range(n):                                               # one chain, k ascending, taps outermost
            chain.addcmul_(Xt[t][:, None], Wm[t][None, :])
    blocked = blocked32(X, Wm)
    P = 1 << max(0, (n - 1).bit_length())
    pair = torch.empty(R, Cc, dtype=F32)
    step = max(1, (1 << 25) // (P * Cc))
    for r0 in range(0, R, step):
        pr = torch.zeros(min(step, R - r0), P, Cc, dtype=F32)
        pr[:, :n] = X[r0:r0 + step, :, None] * Wm[None]
        while pr.shape[1] > 1:
            pr = pr[:, 0::2] + pr[:, 1::2]
        pair[r0:r0 + step] = pr[:, 0]
    return [chain, blocked, pair]


def blocked32(X: torch.Tensor, Wm: torch.Tensor) -> torch.Tensor:
    """float32 sum of one exactly-summed, once-rounded partial per 32-wide k block, blocks in order (an idealised MFMA step)."""
    R, n = X.shape
    nb = (n + 31) // 32
    Xp = torch.zeros(R, nb * 32, dtype=F64)
    Xp[:, :n] = X
    Wp = torch.zeros(nb * 32, Wm.shape[1], dtype=F64)
    Wp[:n] = Wm
    acc = torch.zeros(R, Wm.shape[1], dtype=F32)
    for b in range(nb):
        acc += (Xp[:, b * 32:(b + 1) * 32] @ Wp[b * 32:(b + 1) * 32]).to(F32)
    return acc


def measure_r(Xg: torch.Tensor, Wm: torch.Tensor, seed: int) -> float:
    g = torch.Generator().manual_seed(seed)
    ri = torch.randperm(Xg.shape[0], generator=g)[:R_ORDER_ROWS]
    ci = torch.randperm(Wm.shape[1], generator=g)[:R_ORDER_COLS]
    X, Wc = Xg[ri].to(F64), Wm[:, ci]
    ref, S = X @ Wc, X.abs() @ Wc.abs()
    ok = S > 0
    if not bool(ok.any()):
        return 0.0
    return max(float(((o.to(F64) - ref).abs()[ok] / S[ok]).max()) for o in f32_orders(X, Wc))


def _snake(v, a, err, dt):
    """x + sin^2(a x) / (a + 1e-9) (dac Snake1d as restated in oracle/codec.py) and its error bound."""
    if dt == F32:
        s = torch.sin(a * v)
        return v + (1.0 / (a + torch.tensor(1e-9, dtype=F32))) * (s * s), None
    s = torch.sin(a * v)
    y = v + (s * s) / (a + 1e-9)
    if err is None:
        return y, None
    return y, 2 * err + 2 * s.abs() / a * (SIN_ABS + U * (a * v).abs()) + 4 * U * (v.abs() + s * s / a)


def _erf(x):
    return torch.special.erf(x)


@dataclass
class Out:
    ref: Dict[str, torch.Tensor]                 # kind -> [len(rows), cols]
    err: Dict[str, Optional[torch.Tensor]]
    S: Optional[torch.Tensor] = None             # contractions: sum |x| |w| (times |gamma|), for the record
    r_stage: Optional[float] = None


def eval_stage(st: Stage, env: dict, W: Weights, rows: Optional[torch.Tensor] = None, mode: str = "check") -> Out:
    """ref (and, in mode "check", err) of every buffer `st` writes, on `rows` (default all), from the buffers in env."""
    dt = F32 if mode == "emulate" else F64
    chk = mode == "check"
    rows = torch.arange(st.rows) if rows is None else rows
    p = st.p
    fw = (lambda n: W.f(n).to(dt))

    def carried(C):
        """The rows a stage with a halo reads before row 0: the recorded front rows of a streamed chunk, else an emulated
        bug's stale rows, else None (zeros)."""
        return whole(env[st.src["halo"]], C) if "halo" in st.src else p.get("stale")

    def stores(v, err, alpha_name=None):
        ref, er = {}, {}
        for k in st.dst:
            if k == "act":
                a = fw(alpha_name).reshape(-1)
                a = a.repeat(v.shape[1] // a.numel())
                ref[k], er[k] = _snake(v, a[None, :], err, dt)
            else:
                ref[k], er[k] = v, err
        return ref, er

    if st.kind == "gemm":
        K, N = p["K"], p["N"]
        Wm = pack(st, W)
        if p.get("drop_tap") is not None:                                   # an emulated bug: one tap never accumulated
            Wm = Wm.clone()
            Wm[p["drop_tap"] * K:(p["drop_tap"] + 1) * K] = 0
        Xg = gather(env[st.src["x"]], K, rows, p["offs"], carried(K))
        S = r = E = None
        if mode == "emulate":
            acc = blocked32(Xg.to(F64), Wm)
        else:
            acc = Xg.to(F64) @ Wm
        if chk:
            S = (Xg.to(F32).abs() @ Wm.abs().to(F32)).to(F64) * (1 + 1e-5)    # a float32 product: S only scales a bound
            r = measure_r(Xg, Wm, seed=st.rows * 31 + N)
            E = min(MARGIN * r, Xg.shape[1] * 2.0 ** -23) * S
        n_mod = p["n_mod"]
        rep = (lambda t: t.reshape(-1).repeat(N // n_mod)[None, :])
        v = acc
        err = E
        if p["bias"] and not p.get("drop_bias"):
            v = v + rep(fw(p["bias"]))
            err = err + U * v.abs() if chk else None
        if p["act"] == "gelu":
            g = 0.5 * v * (1.0 + _erf(v * 0.70710678118654752))
            err = 1.13 * err + 0.5 * v.abs() * (LIB + 2 * U) + 2 * U * g.abs() if chk else None
            v = g
        elif p["act"] == "swiglu":
            h = N // 2
            gate, up = v[:, :h], v[:, h:]
            sg = gate / (1.0 + torch.exp(-gate))
            o = sg * up
            if chk:
                eg, eu = err[:, :h], err[:, h:]
                err = up.abs() * (1.1 * eg + (LIB + 3 * U) * sg.abs()) + sg.abs() * eu + 1.1 * eg * eu + U * o.abs()
                S = torch.maximum(S[:, :h], S[:, h:])
            v = o
        if p["gamma"]:
            gm = rep(fw(p["gamma"]))
            v = v * gm
            if chk:
                err = gm.abs() * err + U * v.abs()
                S = S * gm.abs()
        if "resid" in st.src:
            res = gather(env[st.src["resid"]], st.cols, rows, [0]).to(dt)
            v = v + res
            err = err + U * v.abs() if chk else None
        ref, er = stores(v, err, p["alpha"])
        return Out(ref, er, S, r)

    if st.kind == "rvq":
        codes = p["codes"]
        c_sem = W.w["quantizer.semantic_quantizer.quantizers.0.codebook.weight"].shape[0]
        v = torch.zeros(len(rows), st.cols, dtype=dt)
        e1 = torch.zeros(len(rows), st.cols, dtype=F64)
        sabs = torch.zeros(len(rows), st.cols, dtype=F64)
        zr = None
        for i in range(codes.shape[0]):
            q = "quantizer.semantic_quantizer.quantizers.0" if i == 0 else f"quantizer.quantizer.quantizers.{i - 1}"
            cb, w, b = fw(f"{q}.codebook.weight"), fw(f"{q}.out_proj.weight")[:, :, 0], fw(f"{q}.out_proj.bias")
            idx = codes[i, rows].clamp(0, (c_sem if i == 0 else cb.shape[0]) - 1)
            e = cb[idx]
            tab = (cb @ w.t() + b)[idx]           # the whole table, then the rows: as at load time, and the same sums for any row count
            if i == 0:
                zs = tab
            else:
                zr = tab if zr is None else zr + tab
            if chk:
                e1 += (cb.shape[1] + 1) * U * (e.abs() @ w.abs().t() + b.abs())
                sabs += tab.abs()
        v = zs + zr if zr is not None else zs
        err = e1 + codes.shape[0] * U * sabs if chk else None
        return Out(*stores(v, err))

    if st.kind == "rmsnorm":
        x = whole(env[st.src["x"]], st.cols)[rows].to(dt)
        w = fw(p["w"])
        eps = torch.tensor(p.get("eps", 1e-5), dtype=dt)
        v = x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps) * w
        err = (st.cols / 512 + 10) * U * v.abs() if chk else None
        return Out(*stores(v, err))

    if st.kind == "rope":
        H, hd = p["H"], p["hd"]
        x = whole(env[st.src["x"]], st.cols)[rows].to(dt)
        tab = p["tab"][rows + p.get("t0", 0)].to(dt)                        # [R, hd/2, 2]: rows t0 .. of the table
        qk = x[:, :2 * H * hd].reshape(len(rows), 2 * H, hd // 2, 2)
        c, s = tab[:, None, :, 0], tab[:, None, :, 1]
        x0, x1 = qk[..., 0], qk[..., 1]
        re, im = x0 * c - x1 * s, x1 * c + x0 * s
        v = torch.cat([torch.stack([re, im], dim=-1).reshape(len(rows), -1), x[:, 2 * H * hd:]], dim=1)
        err = None
        if chk:
            e = 2 * U * ((x0 * c).abs() + (x1 * s).abs())
            e2 = 2 * U * ((x1 * c).abs() + (x0 * s).abs())
            err = torch.cat([torch.stack([e, e2], dim=-1).reshape(len(rows), -1), torch.zeros_like(x[:, 2 * H * hd:])], dim=1)
        return Out(*stores(v, err))

    if st.kind == "attn":
        H, hd, win = p["H"], p["hd"], p["window"]
        x = whole(env[st.src["x"]], 3 * H * hd).to(dt)
        nh = p.get("nh", 0) if "kv" in st.src else 0                        # carried key / value rows in front of the chunk's
        kv = torch.cat([whole(env[st.src["kv"]], 2 * H * hd).to(dt), x[:, H * hd:]], dim=0) if nh else x[:, H * hd:]
        T = kv.shape[0]
        q = x[:, :H * hd].reshape(-1, H, hd).transpose(0, 1)[:, rows]       # [H, R, hd]
        k, vv = (kv[:, i * H * hd:(i + 1) * H * hd].reshape(T, H, hd).transpose(0, 1) for i in range(2))     # [H, T, hd]
        scale = 1.0 / math.sqrt(hd)
        t = rows[:, None] + nh
        j = torch.arange(T)[None, :]
        bug = p.get("bug")                                                  # emulated faults of the carried form
        lo = (rows[:, None] - win + 1).clamp_min(0) if bug == "window_ignores_nh" else (t - win + 1).clamp_min(0)
        if bug == "drops_oldest" and nh == win - 1:
            lo = lo.clamp_min(1)
        mask = (j <= t) & (j >= lo)                                         # the band of vocoder.py:325-332
        sc = (q @ k.transpose(1, 2)) * scale
        sc = sc.masked_fill(~mask[None], float("-inf"))
        mx = sc.max(dim=-1, keepdim=True).values
        pw = torch.softmax(sc, dim=-1)
        o = pw @ vv
        err = None
        if chk:
            ds = (hd + 2) * U * scale * (q.abs() @ k.abs().transpose(1, 2)) + U * (sc - mx).abs().nan_to_num(posinf=0.0, neginf=0.0)
            Dm = ds.masked_fill(~mask[None], 0.0).max(dim=-1, keepdim=True).values
            nk = mask.sum(dim=-1).to(F64)[None, :, None]
            err = (2 * (Dm + LIB) + (nk + nk / 64 + 12) * U) * (pw @ vv.abs())
            err = err.transpose(0, 1).reshape(len(rows), H * hd)
        v = o.transpose(0, 1).reshape(len(rows), H * hd)
        return Out(*stores(v, err))

    if st.kind == "dwln":
        C = st.cols
        w, b, lw, lb = fw(p["w"])[:, 0, :], fw(p["b"]), fw(p["lw"]), fw(p["lb"])
        xg = gather(env[st.src["x"]], C, rows, [k - 6 for k in range(7)], carried(C)).to(dt).reshape(len(rows), 7, C)
        a = b + (xg * w.t()[None]).sum(dim=1) if dt == F64 else b + sum(xg[:, k] * w[:, k] for k in range(7))
        mean = a.mean(dim=-1, keepdim=True)
        d = a - mean
        var = (d * d).mean(dim=-1, keepdim=True)
        inv = torch.rsqrt(var + torch.tensor(1e-6, dtype=dt))
        v = d * inv * lw + lb
        err = None
        if chk:
            n1 = C / 256 + 10
            ea = 8 * U * (b.abs() + (xg.abs() * w.t().abs()[None]).sum(dim=1))
            dm = ea.mean(dim=-1, keepdim=True) + n1 * U * a.abs().mean(dim=-1, keepdim=True)
            dd = ea + dm + U * d.abs()
            dv = 2 * (d.abs() * dd).mean(dim=-1, keepdim=True) + n1 * U * var
            ri = dv / (2 * (var + 1e-6)) + 3 * U
            err = lw.abs() * inv * (dd + d.abs() * ri) + 3 * U * ((d * inv * lw).abs() + lb.abs())
        return Out(*stores(v, err))

    if st.kind == "final":
        C = p["C"]
        w, b = fw(p["w"])[0], fw(p["b"])                                    # [C][7]
        wm = w.t().reshape(-1, 1)                                           # tap-major [7 C, 1]
        xg = gather(env[st.src["x"]], C, rows, [k - 6 for k in range(7)], carried(C)).to(dt)
        acc = xg @ wm + b
        v = torch.tanh(acc)
        err = None
        if chk:
            S = xg.abs() @ wm.abs() + b.abs()
            err = (7 * max(8, -(-C // 16)) + 6) * U * S + (LIB + U) * v.abs()
        return Out(*stores(v, err))

    if st.kind == "enc_in":
        C = st.cols
        w, b = fw(p["w"])[:, 0, :], fw(p["b"])                              # [C][7]
        xg = gather(p["audio"].reshape(-1, 1), 1, rows, [k - 6 for k in range(7)]).to(dt)    # [R, 7]
        acc = xg @ w.t() + b
        err = 8 * U * (xg.abs() @ w.abs().t() + b.abs()) if chk else None
        return Out(*stores(acc, err, p["alpha"]))

    if st.kind == "snake":
        x = whole(env[st.src["x"]], st.cols)[rows].to(dt)
        return Out(*stores(x, torch.zeros_like(x) if chk else None, p["alpha"]))

    if st.kind in CARRY_KINDS:
        # pure copies, restated on exact values (bf16 patterns survive from_raw / bf16_bits unchanged); bound 0
        bug = p.get("bug")
        if st.kind == "roll":
            H, C = st.rows, st.cols
            x = whole(env[st.src["x"]], C).to(F64)
            prev = whole(env[st.src["prev"]], C).to(F64) if st.src["prev"] in env else torch.zeros(H, C, dtype=F64)
            Tm = x.shape[0]
            cat = torch.cat([prev, x], dim=0)
            carry = cat[-H:].clone()
            if bug == "tail_src_r" and Tm < H:                              # tail_in[r] in place of tail_in[r + T]
                carry[:H - Tm] = prev[:H - Tm]
            if bug == "chunk_only" and Tm < H:                              # rows that should come from the old carry
                carry[:H - Tm] = 0
            ref = {"front": prev, "carry": carry}
        elif st.kind == "kvin":
            prev = whole(env[st.src["prev"]], st.cols).to(F64)
            W1 = p["W1"]
            sh = 1 if bug == "off_by_one" else 0
            ref = {"front": prev[torch.arange(W1 - st.rows, W1) - sh]}
        else:
            HD, W1 = p["HD"], st.rows
            cat = whole(env[st.src["x"]], 3 * HD).to(F64)[:, HD:]
            if "front" in st.src:
                cat = torch.cat([whole(env[st.src["front"]], 2 * HD).to(F64), cat], dim=0)
            n2 = min(W1, cat.shape[0])
            carry = torch.zeros(W1, 2 * HD, dtype=F64)
            carry[W1 - n2:] = cat[-n2:]
            if bug == "writes_all_rows" and n2 < W1:                        # rows that do not exist yet: whatever lies before
                carry[:W1 - n2] = cat[0]
            ref = {"carry": carry}
        ref = {k: v[rows].to(dt) for k, v in ref.items()}
        return Out(ref, {k: (torch.zeros_like(v, dtype=F64) if chk else None) for k, v in ref.items()})

    if st.kind == "tof32":
        x = whole(env[st.src["x"]], st.cols)[rows].to(dt)
        return Out(*stores(x, torch.zeros_like(x) if chk else None))
    raise ValueError(st.kind)


# ------------------------------------------------------------------------------------------------------ chains
def chain_free(plan: List[Stage], weights: Dict[str, torch.Tensor], keep=(), env: Optional[dict] = None) -> dict:
    """The plan in float64 on its own outputs with the unrounded weights; returns the final buffers by logical name and,
    for the stage names in `keep`, what that stage wrote (under the stage's name).  env: the buffers before the first
    launch (a streamed chunk: the carries of the chunk before it)."""
    W, env, kept = Weights(weights, dev=False), dict(env or {}), {}
    for st in plan:
        o = eval_stage(st, env, W, None, "free")
        for k, b in st.dst.items():
            env[b] = o.ref[k]
        if st.name in keep:
            kept[st.name] = o.ref
    env.update(kept)
    return env


def check_trace(plan: List[Stage], trace: List[Dict[str, np.ndarray]], weights: Dict[str, torch.Tensor], seed: int = 0,
                bm: int = 128, env: Optional[dict] = None) -> List["Verdict"]:
    """The checker over a whole trace held in memory (the GPU test does the same in windows of launches).  env: the
    buffers before the first launch (a streamed chunk: the carries recorded for the chunk before it); updated in place."""
    W, env, out = Weights(weights, dev=True), ({} if env is None else env), []
    for st, outs in zip(plan, trace):
        out.append(check_stage(st, env, W, outs, select_rows(st.rows, st.halo, bm, seed)))
        for k, b in st.dst.items():
            env[b] = outs[k]
    return out


def raw_store(kind: str, v: torch.Tensor) -> np.ndarray:
    return v.to(F32).contiguous().numpy() if kind == "f32" else bf16_bits(v)


def chain_emulate(plan: List[Stage], weights: Dict[str, torch.Tensor], override: Optional[Dict[str, Stage]] = None,
                  mutate: Optional[Dict[str, Callable]] = None, env: Optional[dict] = None) -> List[Dict[str, np.ndarray]]:
    """A synthetic trace: every launch in float32 with the device's storage formats, on the outputs before it.
    override[name]: evaluate that launch as another Stage (an emulated bug in its parameters); mutate[name](outs):
    alter what it stored.  Later launches run on the altered values, as they would on the device.  env: the buffers
    before the first launch (a streamed chunk: the carries of the chunk before it); it is updated in place."""
    W, env, trace = Weights(weights, dev=True), ({} if env is None else env), []
    for st in plan:
        o = eval_stage((override or {}).get(st.name, st), env, W, None, "emulate")
        outs = {k: raw_store(k, o.ref[k]) for k in st.dst}
        if mutate and st.name in mutate:
            outs = mutate[st.name](outs)
        for k, b in st.dst.items():
            env[b] = outs[k]
        trace.append(outs)
    return trace


# ------------------------------------------------------------------------------------------------------ the checker
@dataclass
class Verdict:
    name: str
    kind: str
    checked: int = 0
    flagged: int = 0
    rows: List[int] = field(default_factory=list)         # rows with a flagged element
    worst: float = 0.0                                     # largest |got - ref| / bound
    r_stage: Optional[float] = None
    over_S: Optional[float] = None                         # largest |got - ref| / S of an f32-stored contraction


def check_stage(st: Stage, env: dict, W: Weights, got: Dict[str, np.ndarray], rows: Optional[torch.Tensor] = None) -> Verdict:
    """Every element of the checked rows of every buffer the launch wrote, against ref: no element is left out."""
    rows = torch.arange(st.rows) if rows is None else rows
    o = eval_stage(st, env, W, rows, "check")
    v = Verdict(st.name, st.stat_kind, r_stage=o.r_stage)
    assert set(got) == set(st.dst), (st.name, sorted(got), sorted(st.dst))
    bad_rows = torch.zeros(len(rows), dtype=torch.bool)
    for k in st.dst:
        g = from_raw(np.asarray(got[k]).reshape(st.rows, st.cols)[rows.numpy()]).to(F64)
        ref, err = o.ref[k].to(F64), o.err[k]
        assert g.shape == ref.shape == err.shape, (st.name, k, g.shape, ref.shape, err.shape)
        if st.kind in CARRY_KINDS:                          # a copy: the bit patterns themselves
            gb = np.asarray(got[k]).reshape(st.rows, st.cols)[rows.numpy()]
            bad = torch.from_numpy(gb != bf16_bits(o.ref[k]))
            v.checked += bad.numel()
            v.flagged += int(bad.sum())
            bad_rows |= bad.any(dim=1)
            v.worst = max(v.worst, float("inf") if bool(bad.any()) else 0.0)
            continue
        bound = half_ulp(torch.maximum(g.abs(), ref.abs()), k == "f32") + err
        diff = (g - ref).abs()
        bad = ~(diff <= bound)                              # NaN flags
        v.checked += diff.numel()
        v.flagged += int(bad.sum())
        bad_rows |= bad.any(dim=1)
        v.worst = max(v.worst, float((diff / bound).nan_to_num(nan=float("inf")).max()))
        if k == "f32" and o.S is not None:
            ok = o.S > 0
            v.over_S = float((diff[ok] / o.S[ok]).max()) if bool(ok.any()) else 0.0
    v.rows = rows[bad_rows].tolist()
    return v


# ------------------------------------------------------------------------------------------------ the quantiser search
RVQ_B_CAP = 5e-5              # the bound the search was already held to at the real widths (tests/test_codec_gpu.py)
RVQ_NON_ARGMAX_CAP = 0.01     # share of a case's decisions that may be picks other than the float64 argmax (each inside b)


def vq_prefix(q: int) -> str:
    return "quantizer.semantic_quantizer.quantizers.0" if q == 0 else f"quantizer.quantizer.quantizers.{q - 1}"


def first_identical(cb: torch.Tensor) -> torch.Tensor:
    """[N]: for every row of the f32 codebook the lowest index of a row with the same bit pattern."""
    a = np.ascontiguousarray(cb.to(F32).numpy())
    _, first, inv = np.unique(a.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    return torch.from_numpy(first[inv.reshape(-1)].astype(np.int64))


@dataclass
class SearchVerdict:
    """Per decision [codebook, frame]: the bound b, best score - the pick's score, the float64 argmax and runner-up (lowest
    index of their groups of bit-identical rows) and the gap between them; and the lists a test asserts on."""
    b: np.ndarray
    deficit: np.ndarray
    argmax: np.ndarray
    runner: np.ndarray
    gap: np.ndarray
    b_derived_max: float
    outside: List[tuple] = field(default_factory=list)      # (frame, codebook, deficit, b): a pick farther than b from the best
    ties: List[tuple] = field(default_factory=list)         # (frame, codebook, pick, lowest identical row)
    invalid: List[tuple] = field(default_factory=list)      # (frame, codebook, pick): not an index of the codebook

    @property
    def decisions(self) -> int:
        return int(self.b.size)

    @property
    def non_argmax(self) -> int:
        return int((self.deficit > 0).sum())

    @property
    def flagged(self) -> List[tuple]:
        """(frame, codebook) of every faulty decision, sorted."""
        return sorted({(t, q) for t, q, *_ in self.outside + self.ties + self.invalid})

    @property
    def ok(self) -> bool:
        return not self.flagged and self.non_argmax <= RVQ_NON_ARGMAX_CAP * self.decisions

    def summary(self) -> str:
        return (f"{self.decisions} decisions, {self.non_argmax} picks other than the float64 argmax, {len(self.outside)} outside b, "
                f"{len(self.ties)} tie faults, b <= {float(self.b.max()):.2e} (derived up to {self.b_derived_max:.2e}), "
                f"largest deficit / b {float((self.deficit / self.b).max()):.3f}")


def rvq_search_check(shape: OC.CodecShape, weights: Dict[str, torch.Tensor], zq, codes) -> SearchVerdict:
    """Every decision of a quantiser search judged in float64 (the module docstring derives the rule and b): zq (T, D) are
    the pre-quantiser latents the search read (f32, as recorded), codes (1 + n_codebooks, T) the device's picks."""
    W = Weights(weights, dev=False)
    res = from_raw(np.ascontiguousarray(zq, dtype=np.float32)).to(F64)
    codes = torch.as_tensor(np.asarray(codes)).long()
    T, D = res.shape
    R, cd = shape.n_codebooks + 1, shape.codebook_dim
    assert codes.shape == (R, T), (tuple(codes.shape), R, T)
    dres = torch.zeros(T, D, dtype=F64)
    ar = torch.arange(T)
    out = SearchVerdict(*(np.zeros((R, T), dtype=dt) for dt in (np.float64, np.float64, np.int64, np.int64, np.float64)), 0.0)
    for q in range(R):
        p = vq_prefix(q)
        Win, bin_ = W.f(f"{p}.in_proj.weight")[:, :, 0], W.f(f"{p}.in_proj.bias")
        cb, wout, bout = W.f(f"{p}.codebook.weight"), W.f(f"{p}.out_proj.weight")[:, :, 0], W.f(f"{p}.out_proj.bias")
        N = cb.shape[0]
        e = res @ Win.t() + bin_
        de = U * e.abs() + (D / 256 + 12) * 2.0 ** -53 * (res.abs() @ Win.abs().t() + bin_.abs()) + dres @ Win.abs().t()
        ne = e.norm(dim=1).clamp_min(1e-12)
        en = e / ne[:, None]
        cbn = cb / cb.norm(dim=1, keepdim=True).clamp_min(1e-12)
        rep = first_identical(weights[f"{p}.codebook.weight"])
        score = -((en * en).sum(dim=1, keepdim=True) - 2.0 * (en @ cbn.t()) + (cbn * cbn).sum(dim=1)[None, :])
        score = score[:, rep]                                  # bit-identical rows: one value, whatever the order of the sums
        pick = codes[q]
        valid = (pick >= 0) & (pick < N)
        out.invalid += [(int(t), q, int(pick[t])) for t in ar[~valid]]
        pick = pick.clamp(0, N - 1)
        lowest = score.clone()
        lowest[:, rep != torch.arange(N)] = float("-inf")      # one candidate per group of identical rows
        top = lowest.topk(min(2, N), dim=1)
        best = top.values[:, 0]
        deficit = best - score[ar, pick]
        b_derived = 2.0 * ((6 * cd + 33) * U + 4.0 * de.norm(dim=1) / ne)
        b = b_derived.clamp_max(RVQ_B_CAP)
        out.b[q], out.deficit[q], out.argmax[q] = b.numpy(), deficit.numpy(), top.indices[:, 0].numpy()
        out.runner[q], out.gap[q] = top.indices[:, -1].numpy(), (best - top.values[:, -1]).numpy()
        out.b_derived_max = max(out.b_derived_max, float(b_derived.max()))
        far = ~(deficit <= b) & valid                          # NaN flags
        out.outside += [(int(t), q, float(deficit[t]), float(b[t])) for t in ar[far]]
        low = rep[pick]
        out.ties += [(int(t), q, int(pick[t]), int(low[t])) for t in ar[(low != pick) & valid]]
        # the residual the device went on with: minus the table row of ITS pick
        dres = dres + (cd + 1) * U * (cb[pick].abs() @ wout.abs().t() + bout.abs())
        res = res - (cb[pick] @ wout.t() + bout)
        dres = dres + U * res.abs()
    return out


def rvq_search_emulate(shape: OC.CodecShape, weights: Dict[str, torch.Tensor], zq, bug: Optional[dict] = None) -> np.ndarray:
    """An honest float32 stand-in for rvq_encode_kernel (the projection in f64 rounded once to f32, everything after it in
    f32, first index on equal scores), (1 + n_codebooks, T) picks; with `bug`, one emulated fault:
      {"no_update": q}     the residual is not updated after codebook q;
      {"offset": q}        residual codebook q's rows (normalised rows, norms and table) read at the semantic codebook's
                           offset rule, S0 + (q - 1) S0 for S0 + (q - 1) S;
      {"no_bias": q}       the in-projection bias of codebook q dropped;
      {"last_on_ties": 1}  the highest index kept on equal scores;
      {"force": {(t, q): i}}  the pick of frame t at codebook q replaced by row i (the residual follows the replaced pick)."""
    bug = bug or {}
    W = Weights(weights, dev=False)
    res = from_raw(np.ascontiguousarray(zq, dtype=np.float32)).to(F32).clone()
    T = res.shape[0]
    R, S0, S = shape.n_codebooks + 1, shape.semantic_codebook_size, shape.codebook_size
    cbn_all, cn2_all, tab_all = [], [], []
    for q in range(R):                                         # what the load leaves on the device, all codebooks in one array
        p = vq_prefix(q)
        cb = W.f(f"{p}.codebook.weight").to(F32)
        inv = 1.0 / (cb * cb).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
        cn = cb * inv
        cbn_all.append(cn)
        cn2_all.append((cn * cn).sum(dim=1))
        tab_all.append(cb @ W.f(f"{p}.out_proj.weight")[:, :, 0].to(F32).t() + W.f(f"{p}.out_proj.bias").to(F32))
    cbn_all, cn2_all, tab_all = torch.cat(cbn_all), torch.cat(cn2_all), torch.cat(tab_all)
    codes = np.zeros((R, T), dtype=np.int64)
    for q in range(R):
        p = vq_prefix(q)
        N = S0 if q == 0 else S
        off = 0 if q == 0 else S0 + (q - 1) * (S0 if bug.get("offset") == q else S)
        assert off + N <= cbn_all.shape[0], "the emulated offset fault must stay inside the arrays"
        e = res.to(F64) @ W.f(f"{p}.in_proj.weight")[:, :, 0].t()
        if bug.get("no_bias") != q:
            e = e + W.f(f"{p}.in_proj.bias")
        e = e.to(F32)
        inv = 1.0 / (e * e).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
        en = e * inv
        l2 = (en * en).sum(dim=1, keepdim=True)
        dot = torch.zeros(T, N, dtype=F32)
        for k in range(shape.codebook_dim):
            dot = dot + en[:, k:k + 1] * cbn_all[off:off + N, k][None, :]
        score = (-((l2 - 2.0 * dot) + cn2_all[off:off + N][None, :])).numpy()
        pick = N - 1 - np.argmax(score[:, ::-1], axis=1) if bug.get("last_on_ties") else np.argmax(score, axis=1)
        for (t, qq), i in bug.get("force", {}).items():
            if qq == q:
                pick[t] = i
        codes[q] = pick
        if bug.get("no_update") != q:
            res = res - tab_all[off + torch.from_numpy(pick)]
    return codes
