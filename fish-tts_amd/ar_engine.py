"""Host driver of the HIP dual-AR path: the Python side of the S2 seam —
init_model / generate / generate_streaming of fish_tts/models/inference.py:281-414,645-738 — on top
of the C ABI (include/fishtts_hip.h).  torch is used only to hold weight tensors."""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .config import DualARModelArgs


class HipError(RuntimeError):
    pass


logger = logging.getLogger(__name__)


def _rope_table(n_pos: int, n_elem: int, base: float) -> torch.Tensor:
    """cos/sin pairs rounded to bf16, as the reference builds them (llama.py:594-603), returned as f32."""
    expo = torch.arange(0, n_elem, 2)[: n_elem // 2].float() / n_elem
    inv_freq = 1.0 / (base ** expo)
    ang = torch.outer(torch.arange(n_pos), inv_freq)
    z = torch.polar(torch.ones_like(ang), ang)
    return torch.stack([z.real, z.imag], dim=-1).to(torch.bfloat16).float().contiguous()


def normalise_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Key layout handling of llama.py:484-498 and the wq/wk/wv -> wqkv fuse of llama.py:222-227."""
    if "state_dict" in sd:
        sd = sd["state_dict"]
    if next(iter(sd.keys())).startswith("model."):
        sd = {k.replace("model.", ""): v for k, v in sd.items()}
    sd = {k: v for k, v in sd.items() if "audio_" not in k}
    out = dict(sd)
    for k in list(sd.keys()):
        if k.endswith("attention.wq.weight"):
            pre = k[: -len("wq.weight")]
            out[pre + "wqkv.weight"] = torch.cat([out.pop(pre + "wq.weight"), out.pop(pre + "wk.weight"),
                                                  out.pop(pre + "wv.weight")])
    return out


def contiguous_runs(slots: Sequence[int]) -> list:
    """Indices into `slots`, grouped into runs of consecutive slot numbers in ascending slot order: [5, 2, 3, 9] ->
    [[1, 2], [0], [3]] (ft_ar_first_frames draws the first frames of a contiguous slot range in one lock-step pass)."""
    order = sorted(range(len(slots)), key=lambda i: slots[i])
    runs, a = [], 0
    while a < len(order):
        b = a + 1
        while b < len(order) and slots[order[b]] == slots[order[b - 1]] + 1:
            b += 1
        runs.append(order[a:b])
        a = b
    return runs


class ARHipEngine:
    """One GPU context holding the dual-AR weights, KV caches and the captured frame graph.  Batch-1 frames: the
    persistent frame engine (bf16) or launches; lock-step batches of >= 5 rows: five MFMA launches per layer in bf16 and
    fp16, the multi-row GEMV launches in fp32 (frame_path() says which)."""

    def __init__(self, args: DualARModelArgs, semantic_begin_id: int, semantic_end_id: int, im_end_id: int,
                 precision: str = "bf16", device: int = 0, max_batch: int = 1, max_new_tokens: int = 2048,
                 codec_cfg: Optional[L.ft_codec_config] = None):
        if precision not in ("bf16", "fp16", "fp32"):
            raise ValueError(f"precision {precision!r}: expected 'bf16', 'fp16' or 'fp32' (synthesizer.py:122-128)")
        self.args = args
        self.precision = precision
        self.lib = L.load()
        c = L.ft_ar_config()
        c.dtype = {"bf16": L.FT_BF16, "fp16": L.FT_F16, "fp32": L.FT_F32}[precision]
        for name in ("vocab_size", "n_layer", "n_head", "dim", "intermediate_size", "n_local_heads", "head_dim",
                     "max_seq_len", "codebook_size", "num_codebooks", "n_fast_layer", "fast_dim", "fast_n_head",
                     "fast_n_local_heads", "fast_head_dim", "fast_intermediate_size"):
            setattr(c, name, int(getattr(args, name)))
        for name in ("tie_word_embeddings", "attention_qkv_bias", "attention_o_bias", "attention_qk_norm",
                     "scale_codebook_embeddings", "fast_attention_qkv_bias", "fast_attention_qk_norm",
                     "fast_attention_o_bias"):
            setattr(c, name, 1 if getattr(args, name) else 0)
        c.rope_base = float(args.rope_base)
        c.norm_eps = float(args.norm_eps)
        c.semantic_begin_id, c.semantic_end_id, c.im_end_id = int(semantic_begin_id), int(semantic_end_id), int(im_end_id)
        c.max_batch, c.max_new_tokens = int(max_batch), int(max_new_tokens)
        self.cfg = c
        self.R = args.num_codebooks + 1
        self.max_batch = max_batch
        self.max_new_tokens = max_new_tokens
        self.im_end_id = im_end_id
        self._h = C.c_void_p()
        st = self.lib.ft_create(C.byref(c), C.byref(codec_cfg) if codec_cfg is not None else None, device,
                                C.byref(self._h))
        if st != L.FT_OK:
            raise HipError(f"ft_create failed ({st}): {self.lib.ft_last_error(None).decode()}")
        self._loaded = False

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            for pf in list(getattr(self, "_prefixes", [])):
                pf.free()
            self.lib.ft_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int, what: str):
        if st == L.FT_OK:
            return
        msg = self.lib.ft_last_error(self._h).decode()
        if st == L.FT_ERR_TOO_LONG:
            raise ValueError(msg)  # inference.py:296-299
        raise HipError(f"{what} failed ({st}): {msg}")

    # ------------------------------------------------------------------ weights
    def load_tensor(self, name: str, t: torch.Tensor, strict: bool = True) -> bool:
        """Copies one tensor into the library's HBM.  strict=False mirrors the reference's
        load_state_dict(strict=False, assign=True) (llama.py:498) for EXTRA keys only: a name the model does not
        have is skipped (returns False); a wrong shape or rank still raises."""
        t = t.detach()
        if t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            t = t.float()
        t = t.contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        dt = {torch.float32: L.FT_F32, torch.bfloat16: L.FT_BF16, torch.float16: L.FT_F16}[t.dtype]
        st = self.lib.ft_load_weight(self._h, name.encode(), C.c_void_p(t.data_ptr()), dt, shape, t.dim())
        if not strict and st == L.FT_ERR_ARG and self.lib.ft_last_error(self._h).startswith(b"unknown weight name"):
            logger.debug("checkpoint key %s is not a weight of this model: skipped", name)
            return False
        self._check(st, f"ft_load_weight({name})")
        return True

    def load_state_dict(self, sd: Dict[str, torch.Tensor], finalize: bool = True):
        a = self.args
        sd = normalise_state_dict(sd)
        for k, v in sd.items():
            if k.endswith(("freqs_cis", "causal_mask")) or "kv_cache" in k:
                continue
            # extras (an `output.weight` saved beside tied embeddings, `fast_project_in.*` when fast_dim == dim,
            # training-only tensors) are ignored like the reference's strict=False load; a MISSING weight still
            # fails in ft_finalize_weights, a mis-shaped one here
            self.load_tensor(k, v, strict=False)
        self.load_tensor("rope.slow", _rope_table(a.max_seq_len, a.head_dim, a.rope_base))
        self.load_tensor("rope.fast", _rope_table(a.num_codebooks, a.fast_head_dim, a.rope_base))
        if finalize:
            self.finalize()

    def finalize(self):
        self._check(self.lib.ft_finalize_weights(self._h), "ft_finalize_weights")
        self._loaded = True
        logger.info("batch-1 decode frames: %s", self.frame_path())

    def frame_path(self) -> str:
        """Which path the batch-1 frames take (persistent frame engine or launches) and why, then what a lock-step batch
        runs on: "MFMA launches" (bf16 and fp16 at the widths csrc/wide_kernels.h covers, from 5 rows) or the multi-row
        GEMV launches.  batch.run_batch and serve.BatchServer key their 2..4-row rule on that text."""
        return self.lib.ft_ar_frame_path(self._h).decode()

    def inject_engine_fault(self, which: int = 0, workgroup: int = 0, skip: int = 0) -> None:
        """Test hook: a coming slow-stack (0) / codebook-loop (1) engine launch loses one workgroup's rows and times out;
        `skip` launches of that kind pass first."""
        self._check(self.lib.ft_test_engine_fault(self._h, which, workgroup, skip), "ft_test_engine_fault")

    def attn_plan(self):
        """Test hook: (nsplit, xl, n_slots): the KV split count the last prefill / decode call picked, whether the
        slow-stack frame engine is the XCD-local kernel, the rows of the KV cache."""
        n, x, s = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.ft_test_ar_attn_plan(self._h, C.byref(n), C.byref(x), C.byref(s)), "ft_test_ar_attn_plan")
        return n.value, x.value, s.value

    def engine_handoffs(self, which: int, vectors: bool = True, kv=None, tab_row=None):
        """Test hook (ft_test_engine_handoffs): what the frame engine's launches left in their hand-off buffers.  which: 0 the
        slow stack, 1 the codebook loop.  Returns a dict: the geometry words of the hook's struct as ints (copies = 0: that
        engine is off) and, with `vectors` on a context whose engine is on, uint16 (values, tags) pairs x, qkv, xb, g, g3, log
        (loop) or y (slow stack) shaped (copies, 2, layers, n), code (copies, ncb, line) uint32, part / part_tag
        (2, H, nsplit, hd + 2) f32 / uint32.  kv = (layer, slot, rows): also kv_k, kv_v (Hkv, rows, hd) uint16, the slow
        cache (which = 0) or the launch path's codebook-loop cache (which = 1).  tab_row: also tab (QKVN,) uint16, that row
        of the loop's own layer-0 q k v table."""
        io = L.ft_test_engine_io()
        io.which, io.copies = which, 0
        self._check(self.lib.ft_test_engine_handoffs(self._h, C.byref(io)), "ft_test_engine_handoffs")
        geo = ("copies", "epoch", "epoch_step", "n_layer", "D", "QKVN", "HD", "F", "V", "ncb", "H", "Hkv", "hd", "pk3", "pair",
               "qkv0", "resident", "relay", "xl", "nsplit", "line")
        out = {k: int(getattr(io, k)) for k in geo}
        ptr = lambda t: t.ctypes.data_as(C.c_void_p)
        if vectors and io.copies > 0:
            cp, nl = io.copies, io.n_layer
            shapes = dict(x=(nl + 1 if which else 1, io.D), qkv=(nl if which else 1, io.QKVN), xb=(nl if which else 1, io.D),
                          g=(nl if which else 1, io.F))
            if io.pk3:
                shapes["g3"] = shapes["g"]
            shapes["log" if which else "y"] = (1, io.V if which else io.HD)
            for name, (layers, n) in shapes.items():
                v, t = (np.zeros((cp, 2, layers, n), dtype=np.uint16) for _ in range(2))
                out[name], out[name + "_tag"] = v, t
                setattr(io, name, ptr(v)); setattr(io, name + "_tag", ptr(t))
            if which:
                out["code"] = np.zeros((cp, io.ncb, io.line), dtype=np.uint32)
                io.code = ptr(out["code"])
            else:
                out["part"] = np.zeros((2, io.H, io.nsplit, io.hd + 2), dtype=np.float32)
                out["part_tag"] = np.zeros((2, io.H, io.nsplit, io.hd + 2), dtype=np.uint32)
                io.part, io.part_tag = ptr(out["part"]), ptr(out["part_tag"])
        if kv is not None:
            io.kv_layer, io.kv_slot, io.kv_rows = (int(v) for v in kv)
            out["kv_k"], out["kv_v"] = (np.zeros((io.Hkv, io.kv_rows, io.hd), dtype=self._wt()) for _ in range(2))
            io.kv_k, io.kv_v = ptr(out["kv_k"]), ptr(out["kv_v"])
        if tab_row is not None:
            io.tab_row = int(tab_row)
            out["tab"] = np.zeros(io.QKVN, dtype=np.uint16)
            io.tab = ptr(out["tab"])
        if (vectors and io.copies > 0) or kv is not None or tab_row is not None:
            self._check(self.lib.ft_test_engine_handoffs(self._h, C.byref(io)), "ft_test_engine_handoffs")
            out["epoch"] = int(io.epoch)
        return out

    # ------------------------------------------------------------------ primitives
    @staticmethod
    def _sampling(temperature, top_p, repetition_penalty, seed=0, ban_eos=False) -> L.ft_sampling:
        s = L.ft_sampling()
        s.temperature, s.top_p, s.repetition_penalty = float(temperature), float(top_p), float(repetition_penalty)
        s.seed, s.ban_eos = int(seed) & (2 ** 64 - 1), 1 if ban_eos else 0
        return s

    def prefill(self, prompt: np.ndarray, sampling: L.ft_sampling, slot: int = 0, pos0: int = 0) -> np.ndarray:
        """Feeds the (R, Lp) prompt at cache positions [pos0, pos0 + Lp); returns the first generated frame.
        pos0 > 0 continues a restored prefix (kv_restore)."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        assert prompt.ndim == 2 and prompt.shape[0] == self.R, prompt.shape
        out = np.zeros(self.R, dtype=np.int32)
        self._check(self.lib.ft_ar_prefill_at(self._h, slot, prompt.ctypes.data_as(C.c_void_p), prompt.shape[1], pos0,
                                              C.byref(sampling), out.ctypes.data_as(C.c_void_p)), "ft_ar_prefill")
        return out

    def prefill_many(self, prompts: Sequence[np.ndarray], samplings: Sequence[L.ft_sampling], slot0=0,
                     prefixes: Optional[Sequence[Optional["KVPrefix"]]] = None) -> np.ndarray:
        """Prompts of several slots - slot0 = the first of a contiguous range, or the list of (distinct) slots, e.g. the
        ones a scheduler found finished after a burst: the prompt passes in one call (from 5 prompts in bf16 as the rows
        of ONE pass through the slow stack, ft_ar_prefill_slow_many), then the first frames in one lock-step pass per
        contiguous run of slots.  Returns (n, R) first frames in the order of `prompts`."""
        n = len(prompts)
        slots = list(range(slot0, slot0 + n)) if isinstance(slot0, (int, np.integer)) else [int(s) for s in slot0]
        assert len(slots) == n and len(set(slots)) == n, slots
        tails, lps, pos0s = [], np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        for i, prompt in enumerate(prompts):
            prompt = np.ascontiguousarray(prompt, dtype=np.int32)
            assert prompt.ndim == 2 and prompt.shape[0] == self.R, prompt.shape
            pf = prefixes[i] if prefixes is not None else None
            if pf is not None:
                assert 0 < pf.n_pos < prompt.shape[1], (pf.n_pos, prompt.shape)
                self.kv_restore(pf, slots[i])
                pos0s[i], prompt = pf.n_pos, np.ascontiguousarray(prompt[:, pf.n_pos:])
            tails.append(prompt.reshape(-1))
            lps[i] = prompt.shape[1]
        packed = np.ascontiguousarray(np.concatenate(tails)) if n else np.zeros(0, dtype=np.int32)
        slot_arr = np.asarray(slots, dtype=np.int32)
        if n:
            self._check(self.lib.ft_ar_prefill_slow_many(self._h, n, slot_arr.ctypes.data_as(C.c_void_p),
                                                         packed.ctypes.data_as(C.c_void_p), lps.ctypes.data_as(C.c_void_p),
                                                         pos0s.ctypes.data_as(C.c_void_p)), "ft_ar_prefill")
        next_pos = (pos0s + lps).astype(np.int32)
        out = np.zeros((n, self.R), dtype=np.int32)
        for idx in contiguous_runs(slots):             # one lock-step pass per contiguous run of slots
            arr = (L.ft_sampling * len(idx))(*[samplings[i] for i in idx])
            npos = np.ascontiguousarray(next_pos[idx])
            run = np.zeros((len(idx), self.R), dtype=np.int32)
            self._check(self.lib.ft_ar_first_frames(self._h, slots[idx[0]], len(idx), arr, npos.ctypes.data_as(C.c_void_p),
                                                    run.ctypes.data_as(C.c_void_p)), "ft_ar_first_frames")
            out[idx] = run
        return out

    def park(self, slot: int) -> None:
        """Marks a slot idle (finished) for lock-step decoding until its next prefill."""
        self._check(self.lib.ft_ar_park(self._h, slot), "ft_ar_park")

    def move_slot(self, src: int, dst: int) -> None:
        """Moves the live utterance of slot `src` to slot `dst` between decode calls (K/V, frame store, position, ...: one
        launch, ft_ar_slot_move); `src` is left parked.  Its later frames are those it would have drawn in `src`."""
        self._check(self.lib.ft_ar_slot_move(self._h, int(src), int(dst)), "ft_ar_slot_move")

    # ---- reference-prefix K/V reuse
    def kv_save(self, n_pos: int, slot: int = 0) -> "KVPrefix":
        h = C.c_void_p()
        self._check(self.lib.ft_ar_kv_save(self._h, slot, n_pos, C.byref(h)), "ft_ar_kv_save")
        return KVPrefix(self, h, n_pos)

    def kv_restore(self, prefix: "KVPrefix", slot: int = 0) -> None:
        if prefix.engine is not self or not prefix.handle:
            raise ValueError("KV prefix belongs to another engine or was freed")
        self._check(self.lib.ft_ar_kv_restore(self._h, prefix.handle, slot), "ft_ar_kv_restore")

    def build_prefix(self, prefix_cols: np.ndarray, slot: int = 0) -> "KVPrefix":
        """K/V of a prompt prefix (its own prefill; the sampled frame is discarded)."""
        self.prefill(prefix_cols, self._sampling(0.7, 0.7, 1.0), slot)
        return self.kv_save(prefix_cols.shape[1], slot)

    def _start(self, prompt: np.ndarray, sp, prefix: Optional["KVPrefix"], slot: int = 0) -> np.ndarray:
        if prefix is None:
            return self.prefill(prompt, sp, slot)
        assert 0 < prefix.n_pos < prompt.shape[1], (prefix.n_pos, prompt.shape)
        self.kv_restore(prefix, slot)
        return self.prefill(prompt[:, prefix.n_pos:], sp, slot, pos0=prefix.n_pos)

    def decode(self, n_frames: int, samplings: Sequence[L.ft_sampling], poll: int = 8):
        ns = len(samplings)
        arr = (L.ft_sampling * ns)(*samplings)
        frames = np.zeros((ns, max(n_frames, 1), self.R), dtype=np.int32)
        n = np.zeros(ns, dtype=np.int32)
        self._check(self.lib.ft_ar_decode(self._h, ns, n_frames, arr, poll, frames.ctypes.data_as(C.c_void_p),
                                          n.ctypes.data_as(C.c_void_p)), "ft_ar_decode")
        return frames, n

    def set_noise(self, q: Optional[np.ndarray]):
        if q is None:
            self._check(self.lib.ft_ar_set_noise(self._h, None, 0, 0), "ft_ar_set_noise")
            return
        q = np.ascontiguousarray(q, dtype=np.float32)
        self._check(self.lib.ft_ar_set_noise(self._h, q.ctypes.data_as(C.c_void_p), q.shape[0], q.shape[1]),
                    "ft_ar_set_noise")

    def debug_state(self, slot: int = 0):
        logits = np.zeros(self.args.vocab_size, dtype=np.float32)
        hidden = np.zeros(self.args.fast_dim, dtype=np.float32)
        self._check(self.lib.ft_ar_get_debug(self._h, slot, logits.ctypes.data_as(C.c_void_p),
                                             hidden.ctypes.data_as(C.c_void_p)), "ft_ar_get_debug")
        return logits, hidden

    def test_sample(self, logits: np.ndarray, cb: int, sampling: L.ft_sampling, window=None, q=None) -> int:
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        w = None if window is None else np.ascontiguousarray(window, dtype=np.int32)
        qq = None if q is None else np.ascontiguousarray(q, dtype=np.float32)
        out = np.zeros(1, dtype=np.int32)
        self._check(self.lib.ft_test_sample(
            self._h, logits.ctypes.data_as(C.c_void_p), cb, C.byref(sampling),
            None if w is None else w.ctypes.data_as(C.c_void_p),
            None if qq is None else qq.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)), "ft_test_sample")
        return int(out[0])

    DRAW_SENTINEL = 0x7E5A5A5A                                              # integer state a draw must not touch

    def test_draw(self, logits: np.ndarray, cb: int, samplings: Sequence[L.ft_sampling], nf, hist: np.ndarray, last: bool = False,
                  pos=None, done=None, noise=None, omit=None):
        """Test hook (ft_test_draw): ONE draw launch of M = len(logits) rows through the product's own host routine.  logits
        (M, V) f32; nf, pos, done (M,); hist (M, R, cap): each row's history block, whole; noise (rows, row_len) in
        set_noise's layout or None (the counter-based generator).  tokn, tok and rows M .. of every per-row array are
        pre-set to DRAW_SENTINEL (pos, nf, done of rows M ..: too).  Returns a dict of everything the launch could write, max_batch
        rows each: tokn, tok (MB, R), seq (MB, R, cap), pos, nf, done (MB,), femb (MB, fast_dim) f32, qkvf (rows, width) f32,
        xo_femb / xo_x (dim / 8, xo_ldm, 8) uint16 or None, logits (MB, V) (rows M ..: the hook's fill), cut (MB, 8) uint32, chunk_cnt / part_idx
        (MB-row scratch, flat int32), what (see include/fishtts_hip_test.h), path = what & 3.  Nothing is checked here: M, cb and
        last (an int passes as it is) reach the hook, which refuses what is out of range; omit names a pointer left null."""
        a, MB, R, cap = self.args, self.max_batch, self.R, self.max_new_tokens + 24
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        M = logits.shape[0]
        S = self.DRAW_SENTINEL
        ptr = lambda t: None if t is None else t.ctypes.data_as(C.c_void_p)

        def rows(v, shape, fill=S):
            o = np.full((MB,) + shape, fill, dtype=np.int32)
            if v is not None:
                o[:M] = np.asarray(v, dtype=np.int32).reshape((M,) + shape)[:MB]
            return o
        tokn, tok = rows(None, (R,)), rows(None, (R,))
        seq = rows(hist, (R, cap))
        nf_a, pos_a, done_a = rows(nf, ()), rows(np.zeros(M) if pos is None else pos, ()), rows(np.zeros(M) if done is None else done, ())
        fqkv = (a.fast_n_head + 2 * a.fast_n_local_heads) * a.fast_head_dim
        P = 2 * ((MB + 15) // 16 * 16)
        nchunk = (a.vocab_size + 1023) // 1024
        wide = "MFMA launches" in self.frame_path()
        out = dict(logits=np.zeros((MB, logits.shape[1]), dtype=np.float32), femb=np.zeros((MB, a.fast_dim), dtype=np.float32),
                   qkvf=np.zeros((P, fqkv), dtype=np.float32),
                   xo_femb=np.zeros((a.dim // 8, P, 8), dtype=np.uint16) if wide else None,
                   xo_x=np.zeros((a.dim // 8, P, 8), dtype=np.uint16) if wide else None,
                   cut=np.zeros((MB, 8), dtype=np.uint32), chunk_cnt=np.zeros(MB * nchunk, dtype=np.int32),
                   part_idx=np.zeros(MB * nchunk, dtype=np.int32))
        sp = (L.ft_sampling * M)(*samplings)
        q = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
        io = L.ft_test_draw_io()
        io.M, io.cb, io.last, io.what = M, cb, int(last), -1
        io.logits, io.sp, io.noise = ptr(logits), sp, ptr(q)
        io.noise_rows, io.noise_row_len = (0, 0) if q is None else q.shape
        io.tokn, io.tok, io.seq, io.pos, io.nf, io.done = ptr(tokn), ptr(tok), ptr(seq), ptr(pos_a), ptr(nf_a), ptr(done_a)
        io.logits_out, io.femb, io.qkvf = ptr(out["logits"]), ptr(out["femb"]), ptr(out["qkvf"])
        io.xo_femb, io.xo_x = ptr(out["xo_femb"]), ptr(out["xo_x"])
        io.cut, io.chunk_cnt, io.part_idx = ptr(out["cut"]), ptr(out["chunk_cnt"]), ptr(out["part_idx"])
        if omit:
            setattr(io, omit, None)
        self._check(self.lib.ft_test_draw(self._h, C.byref(io)), "ft_test_draw")
        out.update(tokn=tokn, tok=tok, seq=seq, pos=pos_a, nf=nf_a, done=done_a, what=int(io.what), path=int(io.what) & 3)
        return out

    def test_qkv0_tab(self, row0: int, rows: int):
        """Test hook (ft_test_qkv0_tab): rows of the lock-step batches' layer-0 q k v table, (rows, width) uint16, or None."""
        a = self.args
        out = np.zeros((rows, (a.fast_n_head + 2 * a.fast_n_local_heads) * a.fast_head_dim), dtype=np.uint16)
        present = C.c_int32(0)
        self._check(self.lib.ft_test_qkv0_tab(self._h, row0, rows, out.ctypes.data_as(C.c_void_p), C.byref(present)), "ft_test_qkv0_tab")
        return out if present.value else None

    def test_wide_linear(self, epi: int, M: int, X: np.ndarray, W: np.ndarray, gain=None, bias=None, resid=None,
                         alias: bool = False, vocab_head: bool = False):
        """Test hook (ft_test_wide_linear): one Linear of a lock-step batch through the product's dispatcher.  X (M, K),
        W (N, K), gain (K,), resid (M, N): uint16 patterns of the model's type; bias (N,) f32.  Returns (out, tail,
        variant): the M written rows (f32 for epi 0, else uint16), the rows up to the tile edge, the class that ran."""
        u16 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint16)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        X, W, gain, resid = u16(X), u16(W), u16(gain), u16(resid)
        bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        N, K = W.shape
        assert X.shape == (M, K), (X.shape, M, K)
        oc, dt = (N // 2 if epi == 1 else N), (np.float32 if epi == 0 else np.uint16)
        out, tail = np.zeros((M, oc), dtype=dt), np.zeros((31, oc), dtype=dt)
        tr, var = C.c_int32(0), C.c_int32(-1)
        self._check(self.lib.ft_test_wide_linear(self._h, epi, 1 if vocab_head else 0, M, N, K, ptr(X), ptr(W), ptr(gain),
                                                 ptr(bias), ptr(resid), 1 if alias else 0, ptr(out), ptr(tail),
                                                 C.byref(tr), C.byref(var)), "ft_test_wide_linear")
        return out, tail[: tr.value], var.value

    def test_wide_attn(self, qkv: np.ndarray, pos: np.ndarray, qn: np.ndarray, kn: np.ndarray, kc: np.ndarray, vc: np.ndarray):
        """Test hook (ft_test_wide_attn): the slow-stack attention launch of a lock-step batch.  qkv (M, qkvN) f32, pos (M,),
        qn / kn (hd,) and kc / vc (M, Hkv, n_slots, hd) uint16 patterns.  Returns (y (M, H hd) uint16, kc, vc after the
        launch, splits: 0 = attn_wide_kernel, n = the fall-back with n KV splits)."""
        qkv = np.ascontiguousarray(qkv, dtype=np.float32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        qn, kn = np.ascontiguousarray(qn, dtype=np.uint16), np.ascontiguousarray(kn, dtype=np.uint16)
        kc, vc = np.array(kc, dtype=np.uint16, order="C"), np.array(vc, dtype=np.uint16, order="C")     # copies: written in place
        a = self.args
        M = qkv.shape[0]
        n_slots = a.max_seq_len + (-a.max_seq_len) % 8
        assert qkv.shape == (M, (a.n_head + 2 * a.n_local_heads) * a.head_dim), qkv.shape
        assert kc.shape == vc.shape == (M, a.n_local_heads, n_slots, a.head_dim), kc.shape
        y = np.zeros((M, a.n_head * a.head_dim), dtype=np.uint16)
        sp = C.c_int32(-1)
        ptr = lambda t: t.ctypes.data_as(C.c_void_p)
        self._check(self.lib.ft_test_wide_attn(self._h, M, ptr(qkv), ptr(pos), ptr(qn), ptr(kn), ptr(kc), ptr(vc), ptr(y),
                                               C.byref(sp)), "ft_test_wide_attn")
        return y, kc, vc, sp.value

    def test_pf_linear(self, form: int, X: np.ndarray, W: np.ndarray, bias=None, resid=None, alias: bool = False):
        """Test hook (ft_test_pf_linear): one Linear product of the bf16 prompt pass through the product's dispatcher.  form
        0 wqkv, 1 wo / w2 (resid (S, N) f32; alias: in place), 2 w13 (SwiGLU).  X (S, K), W (N, K): bf16 patterns; bias (N,)
        f32.  Returns (out, tail, variant): the S written rows (f32 for forms 0 and 1, else uint16), the rows up to the next
        multiple of 128, the kernel class that ran."""
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        X, W = np.ascontiguousarray(X, dtype=np.uint16), np.ascontiguousarray(W, dtype=np.uint16)
        bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        resid = None if resid is None else np.ascontiguousarray(resid, dtype=np.float32)
        (S, K), N = X.shape, W.shape[0]
        assert W.shape == (N, K) and (resid is None or resid.shape == (S, N)), (X.shape, W.shape)
        oc, dt = (N // 2 if form == 2 else N), (np.uint16 if form == 2 else np.float32)
        out, tail = np.zeros((S, oc), dtype=dt), np.zeros((127, oc), dtype=dt)
        tr, var = C.c_int32(0), C.c_int32(-1)
        self._check(self.lib.ft_test_pf_linear(self._h, form, S, N, K, ptr(X), ptr(W), ptr(bias), ptr(resid), 1 if alias else 0,
                                               ptr(out), ptr(tail), C.byref(tr), C.byref(var)), "ft_test_pf_linear")
        return out, tail[: tr.value], var.value

    def test_pf_norm(self, x: np.ndarray, gain: np.ndarray):
        """Test hook (ft_test_pf_norm): the row RMSNorm of the prompt pass.  x (S, D) f32, gain (D,) bf16 patterns.  Returns
        (out (S, D) uint16, the row behind it)."""
        x, gain = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(gain, dtype=np.uint16)
        S, D = x.shape
        out, tail = np.zeros((S, D), dtype=np.uint16), np.zeros(D, dtype=np.uint16)
        ptr = lambda t: t.ctypes.data_as(C.c_void_p)
        self._check(self.lib.ft_test_pf_norm(self._h, S, D, ptr(x), ptr(gain), ptr(out), ptr(tail)), "ft_test_pf_norm")
        return out, tail

    def test_pf_attn(self, qkv: np.ndarray, qn: np.ndarray, kn: np.ndarray, kc: np.ndarray, vc: np.ndarray, seqs=None,
                     pos0: int = 0, slot: int = 0):
        """Test hook (ft_test_pf_attn): the K/V append and the causal attention of one layer of a prompt pass.  qkv (S, qkvN)
        f32; qn / kn (hd,), kc / vc (max_batch, Hkv, n_slots, hd): bf16 patterns; seqs: None = one prompt of S rows at pos0 of
        `slot`, else (n, 4) int32 {first row, rows, first cache position, slot}.  Returns (y, q (S, H hd) uint16, kc, vc as
        the hook filled them and the pass left them, tail (2, H hd), path: NG of the tiled kernel or 0)."""
        qkv = np.ascontiguousarray(qkv, dtype=np.float32)
        qn, kn = np.ascontiguousarray(qn, dtype=np.uint16), np.ascontiguousarray(kn, dtype=np.uint16)
        kc, vc = np.array(kc, dtype=np.uint16, order="C"), np.array(vc, dtype=np.uint16, order="C")     # copies: written in place
        a = self.args
        S = qkv.shape[0]
        n_slots = a.max_seq_len + (-a.max_seq_len) % 8
        assert qkv.shape == (S, (a.n_head + 2 * a.n_local_heads) * a.head_dim), qkv.shape
        assert kc.shape == vc.shape == (self.max_batch, a.n_local_heads, n_slots, a.head_dim), kc.shape
        sq = None if seqs is None else np.ascontiguousarray(seqs, dtype=np.int32).reshape(-1, 4)
        y, q = (np.zeros((S, a.n_head * a.head_dim), dtype=np.uint16) for _ in range(2))
        tail = np.zeros((2, a.n_head * a.head_dim), dtype=np.uint16)
        path = C.c_int32(-1)
        ptr = lambda t: None if t is None else t.ctypes.data_as(C.c_void_p)
        self._check(self.lib.ft_test_pf_attn(self._h, 0 if sq is None else sq.shape[0], ptr(sq), S, pos0, slot, ptr(qkv), ptr(qn),
                                             ptr(kn), ptr(kc), ptr(vc), ptr(y), ptr(q), ptr(tail), C.byref(path)), "ft_test_pf_attn")
        return y, q, kc, vc, tail, path.value

    def _wt(self):
        """numpy dtype of the patterns the context's weights travel as: uint16 (bf16 / fp16) or float32."""
        return np.float32 if self.precision in ("fp32", "f32") else np.uint16

    def test_gemv(self, pro: int, epi: int, x: np.ndarray, W: np.ndarray, gain=None, bias=None, resid=None, alias: bool = False,
                  nt: bool = True, ldx=None, ldo=None):
        """Test hook (ft_test_gemv): one product of a decode launch of 1..max_batch rows through the product's dispatcher.  x (M, K) f32;
        W (N, K), gain (K,), bias (N,): patterns of the model's type (float32 in fp32); resid (M, N) f32.  Returns (out (M, oc)
        f32, pad (M, ldo - oc) uint32, tail (ldo,) uint32: the row behind, (MB, R, NT))."""
        wt = self._wt()
        c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        x, W, gain, bias, resid = c(x, np.float32), c(W, wt), c(gain, wt), c(bias, wt), c(resid, np.float32)
        (M, K), N = x.shape, W.shape[0]
        oc = N // 2 if epi == 2 else N
        ldx = K if ldx is None else ldx
        ldo = oc + (-oc) % 4 if ldo is None else ldo
        out = np.zeros((M + 1, max(ldo, 1)), dtype=np.float32)
        ids = np.zeros(3, dtype=np.int32)
        self._check(self.lib.ft_test_gemv(self._h, pro, epi, M, N, K, ptr(x), ldx, ptr(W), ptr(gain), ptr(bias), ptr(resid),
                                          1 if alias else 0, 1 if nt else 0, ldo, ptr(out), ptr(ids)), "ft_test_gemv")
        return out[:M, :oc].copy(), out[:M, oc:].view(np.uint32).copy(), out[M].view(np.uint32).copy(), tuple(int(i) for i in ids)

    def test_decode_attn(self, qkv: np.ndarray, pos: np.ndarray, qn, kn, kc: np.ndarray, vc: np.ndarray, wo: np.ndarray, bo,
                         resid: np.ndarray, pos_off: int = 0):
        """Test hook (ft_test_decode_attn): decode attention and the Wo product of 1..max_batch rows.  Patterns of the model's type
        (float32 in fp32) for qn, kn, kc, vc (M, Hkv, n_slots, hd), wo (dim, H hd), bo.  Returns (nsplit, y (M, y_ld) f32,
        part_o (M, H, nsplit, hd), part_ml (M, H, nsplit, 2) or None with one split, x_out (M, dim), kc, vc after the launch)."""
        wt = self._wt()
        c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        a = self.args
        qkv, pos, resid = c(qkv, np.float32), c(pos, np.int32), c(resid, np.float32)
        qn, kn, wo, bo = c(qn, wt), c(kn, wt), c(wo, wt), c(bo, wt)
        kc, vc = np.array(kc, dtype=wt, order="C"), np.array(vc, dtype=wt, order="C")                   # copies: written in place
        M, H, hd = qkv.shape[0], a.n_head, a.head_dim
        n_slots = a.max_seq_len + (-a.max_seq_len) % 8
        y_ld = max(H * hd, a.fast_n_head * a.fast_head_dim)
        assert qkv.shape == (M, (H + 2 * a.n_local_heads) * hd), qkv.shape
        assert kc.shape == vc.shape == (M, a.n_local_heads, n_slots, hd), kc.shape
        assert wo.shape == (a.dim, H * hd) and resid.shape == (M, a.dim), (wo.shape, resid.shape)
        y = np.zeros((M, y_ld), dtype=np.float32)
        po, pm = np.zeros((M * H * 32 * hd,), dtype=np.float32), np.zeros((M * H * 32 * 2,), dtype=np.float32)
        xo = np.zeros((M, a.dim), dtype=np.float32)
        ns = C.c_int32(0)
        self._check(self.lib.ft_test_decode_attn(self._h, M, ptr(qkv), ptr(pos), pos_off, ptr(qn), ptr(kn), ptr(kc), ptr(vc), ptr(wo),
                                                 ptr(bo), ptr(resid), C.byref(ns), ptr(y), ptr(po), ptr(pm), ptr(xo)),
                    "ft_test_decode_attn")
        n = ns.value
        if n > 1:
            po, pm = po[:M * H * n * hd].reshape(M, H, n, hd), pm[:M * H * n * 2].reshape(M, H, n, 2)
        else:
            po = pm = None
        return n, y, po, pm, xo, kc, vc

    def test_embed(self, emb: np.ndarray, cb_emb: np.ndarray, toks: np.ndarray, M: int, ncb: int, cbsize: int, sem_begin: int,
                   sem_end: int, scale: bool, tok_row_stride: int, tok_m_stride: int, ldx=None, xo_ldm: int = 0):
        """Test hook (ft_test_embed): one embed_kernel launch on caller tables.  emb (vocab, D), cb_emb (ncb cbsize, D):
        patterns of the model's type; toks: flat int32.  Returns (x (M, D) f32, pad (M, ldx - D) uint32, tail (ldx,) uint32,
        xo (D / 8, xo_ldm, 8) uint16 or None)."""
        wt = self._wt()
        emb, cb_emb = np.ascontiguousarray(emb, dtype=wt), np.ascontiguousarray(cb_emb, dtype=wt)
        toks = np.ascontiguousarray(toks, dtype=np.int32).reshape(-1)
        vocab, D = emb.shape
        assert cb_emb.shape == (ncb * cbsize, D), cb_emb.shape
        ldx = D if ldx is None else ldx
        x = np.zeros((M + 1, ldx), dtype=np.float32)
        xo = np.zeros(((D + 7) // 8, xo_ldm, 8), dtype=np.uint16) if xo_ldm > 0 else None
        ptr = lambda t: None if t is None else t.ctypes.data_as(C.c_void_p)
        self._check(self.lib.ft_test_embed(self._h, M, D, ncb, cbsize, vocab, ptr(emb), ptr(cb_emb), ptr(toks), toks.size,
                                           tok_row_stride, tok_m_stride, sem_begin, sem_end, 1 if scale else 0, ldx, xo_ldm, ptr(x),
                                           ptr(xo)), "ft_test_embed")
        return x[:M, :D].copy(), x[:M, D:].view(np.uint32).copy(), x[M].view(np.uint32).copy(), xo

    def test_fast_attn(self, form: int, qkv: np.ndarray, c: int, qn, kn, kc: np.ndarray, vc: np.ndarray):
        """Test hook (ft_test_fast_attn): one fast_attn_kernel launch.  form 0 single (M <= max_batch), 1 wide single, 2 paired (qkv
        rows [0, M) at position 0, [M, 2 M) at position 1).  kc / vc (M, Hkv, ncb, hd).  Returns (y, pad, tail, kc, vc) for
        form 0 (y (M, H hd) f32) or (y_bf (H hd / 8, xo_ldm, 8) uint16, kc, vc) for the wide forms; the caches as the hook
        filled them (NaN from row c / 0 on) and the launch left them."""
        wt = self._wt()
        a = self.args
        qkv = np.ascontiguousarray(qkv, dtype=np.float32)
        cc = lambda t: None if t is None else np.ascontiguousarray(t, dtype=wt)
        ptr = lambda t: None if t is None else t.ctypes.data_as(C.c_void_p)
        qn, kn = cc(qn), cc(kn)
        kc, vc = np.array(kc, dtype=wt, order="C"), np.array(vc, dtype=wt, order="C")
        M = qkv.shape[0] // 2 if form == 2 else qkv.shape[0]
        H, hd = a.fast_n_head, a.fast_head_dim
        assert qkv.shape[1] == (H + 2 * a.fast_n_local_heads) * hd, qkv.shape
        assert kc.shape == vc.shape == (M, a.fast_n_local_heads, a.num_codebooks, hd), kc.shape
        y_ld = max(a.n_head * a.head_dim, H * hd)
        y = np.zeros((M + 1, y_ld), dtype=np.float32) if form == 0 else None
        xo_ldm = 2 * ((self.max_batch + 15) // 16 * 16)
        yb = None if form == 0 else np.zeros((H * hd // 8, xo_ldm, 8), dtype=np.uint16)
        self._check(self.lib.ft_test_fast_attn(self._h, form, M, c, ptr(qkv), ptr(qn), ptr(kn), ptr(kc), ptr(vc), ptr(y), ptr(yb)),
                    "ft_test_fast_attn")
        if form == 0:
            return y[:M, :H * hd].copy(), y[:M, H * hd:].view(np.uint32).copy(), y[M].view(np.uint32).copy(), kc, vc
        return yb, kc, vc

    # ------------------------------------------------------------------ launch trace of a frame (test hook)
    def trace_arm(self, first: int = 0, count: int = 1 << 30) -> None:
        """Test hook (ft_test_ar_trace_arm): the next decode(1, ...), first-frames or prompt call (prefill, prefill_slow,
        prefill_slow_many) records one entry per launch; the entries [first, first + count) keep host copies of every buffer
        they wrote."""
        self._check(self.lib.ft_test_ar_trace_arm(self._h, first, count), "ft_test_ar_trace_arm")

    def trace_read(self):
        """Test hook: the last traced call as a dict: kind (1 a decode frame, 2 first frames, 3 prefill, 4 prefill_slow, 5
        prefill_slow_many), m0, M, launches - a list of dicts name, m0, rows, cols, cls (4 ints), pos_off, held, bufs {buffer id:
        array} (f32 / int32 (rows, cols); the octet-major 16-bit buffers as uint16 (width / 8, xo_ldm, 8); the prompt workspace's
        16-bit rows, ids 25 .. 28, as uint16 (max_seq_len, width)) - and state: [before, after], each a dict tok (MB, R), pos, nf, done (MB,),
        seq (MB, R, cap); begin: {buffer id: array}, every traceable buffer as the call found it.  The copies are handed over:
        a second read finds none."""
        info = np.zeros(5, dtype=np.int32)
        n = self.lib.ft_test_ar_trace_count(self._h, info.ctypes.data_as(C.c_void_p))
        if n < 0:
            raise HipError("the launch trace failed to copy a buffer")
        MB, R, cap = self.max_batch, self.R, self.max_new_tokens + 24
        launches = []
        name, li, bi = C.create_string_buffer(64), np.zeros(10, dtype=np.int32), np.zeros(4, dtype=np.int32)
        for i in range(-1, n):
            if i < 0:                                   # the record before the first launch: every buffer as the call found it
                rec = dict(name="begin", m0=0, rows=0, cols=0, held=True, cls=(-1,) * 4, pos_off=0, bufs={})
                li[3] = info[4]
            else:
                self._check(self.lib.ft_test_ar_trace_launch(self._h, i, name, 64, li.ctypes.data_as(C.c_void_p)), "ft_test_ar_trace_launch")
                rec = dict(name=name.value.decode(), m0=int(li[0]), rows=int(li[1]), cols=int(li[2]), held=bool(li[4]),
                           cls=tuple(int(v) for v in li[5:9]), pos_off=int(li[9]), bufs={})
            for j in range(int(li[3])):
                self._check(self.lib.ft_test_ar_trace_buffer(self._h, i, j, bi.ctypes.data_as(C.c_void_p), None), "ft_test_ar_trace_buffer")
                bid, esz, rows, cols = (int(v) for v in bi)
                if not rec["held"]:
                    rec["bufs"][bid] = None
                    continue
                a = np.zeros((rows, cols), dtype=np.uint16 if esz == 2 else np.int32 if bid >= 30 else np.float32)
                self._check(self.lib.ft_test_ar_trace_buffer(self._h, i, j, bi.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)),
                            "ft_test_ar_trace_buffer")
                rec["bufs"][bid] = a.reshape(rows, cols // 8, 8) if esz == 2 and not 25 <= bid <= 28 else a
            if i < 0:
                begin = rec["bufs"]
                continue
            launches.append(rec)
        state = []
        for which in (0, 1):
            s = dict(tok=np.zeros((MB, R), dtype=np.int32), pos=np.zeros(MB, dtype=np.int32), nf=np.zeros(MB, dtype=np.int32),
                     done=np.zeros(MB, dtype=np.int32), seq=np.zeros((MB, R, cap), dtype=np.int32))
            self._check(self.lib.ft_test_ar_trace_state(self._h, which, *(s[k].ctypes.data_as(C.c_void_p) for k in ("tok", "pos", "nf", "done", "seq"))),
                        "ft_test_ar_trace_state")
            state.append(s)
        return dict(kind=int(info[0]), m0=int(info[1]), M=int(info[2]), launches=launches, state=state, begin=begin)

    def read_caches(self):
        """Test hook: every K/V cache of the launch path, whole: {("slow" | "fast", layer): (k, v)}, each (max_batch, Hkv,
        rows, hd) in the context's type (uint16 patterns or float32), rows = the cache's (n_slots / num_codebooks)."""
        a = self.args
        out = {}
        for which, kind, nl, rows in ((0, "slow", a.n_layer, a.max_seq_len + (-a.max_seq_len) % 8), (1, "fast", a.n_fast_layer, a.num_codebooks)):
            for li in range(nl):
                d = [self.engine_handoffs(which, vectors=False, kv=(li, m, rows)) for m in range(self.max_batch)]
                out[(kind, li)] = (np.stack([x["kv_k"] for x in d]), np.stack([x["kv_v"] for x in d]))
        return out

    def test_slots(self, kv: bool = True) -> dict:
        """Test hook (ft_test_ar_slots): the per-slot state of every slot as a dict: geo (the hook's ten geometry words by
        name), tok, tokn (MB, R), pos, nf, done (MB,), seq (MB, R, cap) int32, ctl (MB, ctl_words) uint32, hid_in_xo (MB,)
        uint8 and, with `kv`, kv (n_layer, 2, MB, Hkv, n_slots, head_dim x esz) uint8: the slow caches' bytes."""
        g = np.zeros(10, dtype=np.int32)
        self._check(self.lib.ft_test_ar_slots(self._h, g.ctypes.data_as(C.c_void_p), *([None] * 9)), "ft_test_ar_slots")
        names = ("max_batch", "R", "cap", "ctl_words", "n_layer", "Hkv", "n_slots", "head_dim", "esz", "im_end_id")
        geo = {k: int(v) for k, v in zip(names, g)}
        MB, R, cap = geo["max_batch"], geo["R"], geo["cap"]
        out = dict(tok=np.zeros((MB, R), dtype=np.int32), tokn=np.zeros((MB, R), dtype=np.int32), pos=np.zeros(MB, dtype=np.int32),
                   nf=np.zeros(MB, dtype=np.int32), done=np.zeros(MB, dtype=np.int32), seq=np.zeros((MB, R, cap), dtype=np.int32),
                   ctl=np.zeros((MB, geo["ctl_words"]), dtype=np.uint32), hid_in_xo=np.zeros(MB, dtype=np.uint8))
        if kv:
            out["kv"] = np.zeros((geo["n_layer"], 2, MB, geo["Hkv"], geo["n_slots"], geo["head_dim"] * geo["esz"]), dtype=np.uint8)
        ptr = lambda k: out[k].ctypes.data_as(C.c_void_p) if k in out else None
        self._check(self.lib.ft_test_ar_slots(self._h, None, *(ptr(k) for k in ("tok", "tokn", "pos", "nf", "done", "seq", "ctl",
                                                                               "hid_in_xo", "kv"))), "ft_test_ar_slots")
        out["geo"] = geo
        return out

    def first_frames(self, slot0: int, samplings: Sequence[L.ft_sampling], next_pos) -> np.ndarray:
        """ft_ar_first_frames alone: the first frames of slots [slot0, slot0 + n) whose prompts went through the slow stack."""
        n = len(samplings)
        arr = (L.ft_sampling * n)(*samplings)
        npos = np.ascontiguousarray(next_pos, dtype=np.int32)
        out = np.zeros((n, self.R), dtype=np.int32)
        self._check(self.lib.ft_ar_first_frames(self._h, slot0, n, arr, npos.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)),
                    "ft_ar_first_frames")
        return out

    def prefill_slow_many(self, prompts: Sequence[np.ndarray], slots: Sequence[int], pos0s=None) -> np.ndarray:
        """ft_ar_prefill_slow_many alone: the prompt passes of `slots` (pos0s: behind restored prefixes), no first frames.
        Returns each slot's next position."""
        tails = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in prompts]
        lps = np.asarray([np.asarray(p).shape[1] for p in prompts], dtype=np.int32)
        packed, sl = np.ascontiguousarray(np.concatenate(tails)), np.asarray(slots, dtype=np.int32)
        z = np.zeros(len(prompts), dtype=np.int32) if pos0s is None else np.ascontiguousarray(pos0s, dtype=np.int32)
        self._check(self.lib.ft_ar_prefill_slow_many(self._h, len(prompts), sl.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p),
                                                     lps.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)), "ft_ar_prefill")
        return (lps + z).astype(np.int32)

    def prefill_slow(self, prompt: np.ndarray, slot: int = 0, pos0: int = 0) -> None:
        """ft_ar_prefill_slow alone: one prompt pass, no first frame."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        assert prompt.ndim == 2 and prompt.shape[0] == self.R, prompt.shape
        self._check(self.lib.ft_ar_prefill_slow(self._h, slot, prompt.ctypes.data_as(C.c_void_p), prompt.shape[1], pos0), "ft_ar_prefill_slow")

    def engine_state(self):
        """(flags, time-outs recovered so far, phase of the last one) of the persistent frame engine: flags bit 0 = slow
        stack, bit 1 = fast loop."""
        f, a, w = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self.lib.ft_ar_engine_state(self._h, C.byref(f), C.byref(a), C.byref(w)), "ft_ar_engine_state")
        return f.value, a.value, w.value

    def sync(self):
        self._check(self.lib.ft_sync(self._h), "ft_sync")

    def profile_gemv(self, frames: int, sampling: L.ft_sampling):
        ms, n, b = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self.lib.ft_ar_profile_gemv(self._h, frames, C.byref(sampling), C.byref(ms), C.byref(n),
                                                C.byref(b)), "ft_ar_profile_gemv")
        return ms.value, n.value, b.value

    # ------------------------------------------------------------------ generate (inference.py:281-384)
    def profile_frame(self, frames: int, sampling: L.ft_sampling):
        """(ms of `frames` graph replays, [ms slow stack, ms head + draw, ms fast loop] over frames-1 eager frames,
        launches per captured frame) - slot 0 must be prefilled."""
        ms, n = C.c_double(0), C.c_int32(0)
        seg = (C.c_double * 3)()
        self._check(self.lib.ft_ar_profile_frame(self._h, frames, C.byref(sampling), C.byref(ms), seg, C.byref(n)),
                    "ft_ar_profile_frame")
        return ms.value, [seg[0], seg[1], seg[2]], n.value

    def _clamp_new(self, T: int, max_new_tokens: int) -> int:
        m = self.args.max_seq_len
        if T >= m:
            raise ValueError(f"Input sequence length {T} exceeds max_seq_len {m}")
        if max_new_tokens:
            if T + max_new_tokens > m:
                max_new_tokens = m - T
        else:
            max_new_tokens = m - T
        return min(max_new_tokens, self.max_new_tokens)

    def generate(self, prompt: np.ndarray, max_new_tokens: int, temperature: float = 0.7, top_p: float = 0.7,
                 repetition_penalty: float = 1.5, seed: int = 0, ban_eos: bool = False, poll: int = 8,
                 prefix: Optional["KVPrefix"] = None) -> np.ndarray:
        """(R, T) int32 prompt -> (R, T + n) int32, n <= max_new_tokens, stopping after <|im_end|>.
        `prefix`: saved K/V of the first prefix.n_pos prompt columns (only the rest is prefilled)."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        T = prompt.shape[1]
        n_new = self._clamp_new(T, max_new_tokens)
        sp = self._sampling(temperature, top_p, repetition_penalty, seed, ban_eos)
        first = self._start(prompt, sp, prefix)
        frames, n = self.decode(n_new - 1, [sp], poll)
        return np.concatenate([prompt, first[:, None], frames[0, : n[0]].T], axis=1)

    def generate_streaming(self, prompt: np.ndarray, max_new_tokens: int, temperature: float = 0.7,
                           top_p: float = 0.7, repetition_penalty: float = 1.5, seed: int = 0,
                           ban_eos: bool = False, chunk: int = 8,
                           prefix: Optional["KVPrefix"] = None) -> Iterator[np.ndarray]:
        """Yields (num_codebooks, k) code blocks as they are produced, <|im_end|> frame included
        (inference.py:645-738, 218-276); `chunk` frames per graph burst."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        n_new = self._clamp_new(prompt.shape[1], max_new_tokens)
        sp = self._sampling(temperature, top_p, repetition_penalty, seed, ban_eos)
        first = self._start(prompt, sp, prefix)
        yield first[1:, None]
        left = n_new - 1
        while left > 0:
            k = min(chunk, left)
            frames, n = self.decode(k, [sp], poll=k)
            if n[0] > 0:
                yield frames[0, : n[0], 1:].T
            left -= k
            if n[0] < k or (n[0] > 0 and frames[0, n[0] - 1, 0] == self.im_end_id):
                break


class KVPrefix:
    """Device-resident K/V of the first n_pos prompt positions (one per voice); freed with the engine."""

    def __init__(self, engine: ARHipEngine, handle, n_pos: int):
        self.engine, self.handle, self.n_pos = engine, handle, n_pos
        if not hasattr(engine, "_prefixes"):
            engine._prefixes = []
        engine._prefixes.append(self)

    def free(self) -> None:
        if self.handle:
            self.engine.lib.ft_ar_kv_free(self.engine._h, self.handle)
            self.handle = None
        if self in getattr(self.engine, "_prefixes", []):
            self.engine._prefixes.remove(self)
