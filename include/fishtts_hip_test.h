/* Test and measurement hooks of libfishtts_hip.so - NOT part of the drop-in boundary (include/fishtts_hip.h).
 * Nothing in the product path (fish-tts_amd/*.py outside ARHipEngine's test helpers) calls them: tests/ use them to
 * inject noise, read logits back and provoke the frame engine's recovery; bench.py uses the two profile calls. */
#ifndef FISHTTS_HIP_TEST_H
#define FISHTTS_HIP_TEST_H
#include "fishtts_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test hooks: inject the Exp(1) noise the sampler divides by (inference.py:26), one row of
 * `row_len` floats per generated frame (slow vocab draws first, then (num_codebooks-1) x 1024);
 * q == NULL restores the RNG.  Read back the last slow logits / pre-norm hidden of a slot (after a frame on the lock-step
 * MFMA launches the hidden state is gathered from the octet-major residual stream, where those launches keep it).  Both
 * rows belong to the slot index, not to the utterance: ft_ar_slot_move carries neither them nor the host's note of where
 * the hidden row lies, so after a move they are defined for `to` only once its next frame has run. */
ft_status ft_ar_set_noise(ft_ctx* ctx, const float* q, int64_t n_rows, int64_t row_len);
ft_status ft_ar_get_debug(ft_ctx* ctx, int32_t slot, float* logits /*vocab*/, float* hidden /*fast_dim*/);

/* Test hook: the residual vector quantiser search alone on given pre-quantiser latents z [T][latent_dim] f32 (host). */
ft_status ft_codec_rvq_encode(ft_ctx* ctx, const float* z, int32_t T, int32_t* codes);

/* Measurement hook used by bench.py (never by the product path).  The weight-streaming GEMV launches of
 * one decode frame whose weights come from HBM (4 per slow layer + the vocabulary head; the fast stack's
 * 100 MB stay cache-resident and are excluded) are captured into a hipGraph and replayed `frames` times
 * between two HIP events on the engine's own stream.  Returns the elapsed device ms, the number of kernel
 * launches timed and the algorithmic bytes those launches stream. */
ft_status ft_ar_profile_gemv(ft_ctx* ctx, int32_t frames, const ft_sampling* sp, double* ms,
                             int64_t* launches, int64_t* bytes);
/* Measurement hook used by bench.py (never by the product path): `frames` real decode frames of slot 0 (prefilled by
 * the caller, enough frame / cache capacity left) timed with HIP events on the engine's own stream.
 * ms_graph: elapsed ms of `frames` back-to-back replays of the captured frame graph (what ft_ar_decode runs);
 * seg_ms[3]: ms summed over frames-1 further frames launched eagerly with events between the three parts of a frame:
 * the slow stack, the vocabulary head + semantic draw, the fast codebook loop (bf16 only, else zeros);
 * nodes_per_frame: launches in the captured frame.  Reference: one decode_one_token_ar call, inference.py:83-155. */
ft_status ft_ar_profile_frame(ft_ctx* ctx, int32_t frames, const ft_sampling* sp, double* ms_graph,
                              double* seg_ms, int32_t* nodes_per_frame);

/* Test hook: workgroup `wg` of a coming slow-stack (which = 0) or codebook-loop (which = 1) engine launch publishes
 * nothing, so the launch times out (one shot); `skip` launches of that kind pass first (a later burst of a call, a
 * launch inside a multi-frame graph).  Exercises the recovery described above. */
ft_status ft_test_engine_fault(ft_ctx* ctx, int32_t which, int32_t wg, int32_t skip);

/* Test hook (reads host fields only; no device work, nothing on the frame path): what the slow-stack attention of the LAST
 * ft_ar_prefill / ft_ar_decode call on this context ran on.  *nsplit: the KV split count that call picked (launches and
 * frame engine alike); *xl: 1 if the slow-stack frame engine is on and is the XCD-local kernel (one kv head per XCD), else 0;
 * *n_slots: the rows of the KV cache (max_seq_len rounded up to 8).  Any pointer may be NULL. */
ft_status ft_test_ar_attn_plan(ft_ctx* ctx, int32_t* nsplit, int32_t* xl, int32_t* n_slots);

/* Test hook (host code only: it synchronises the context's stream and copies device memory out; no kernel, no branch in a
 * kernel, nothing on the frame path): everything an utterance owns between two launches, for ALL max_batch slots, so that
 * the calls which carry that state - ft_ar_slot_move, ft_ar_park, ft_ar_reset, ft_ar_kv_save / ft_ar_kv_restore and the
 * ft_ar_prefill_at behind a restore - can be held to "a defined set of bytes is equal, every other byte is untouched".
 * Any pointer may be NULL.
 *   geo [10]: max_batch, R = num_codebooks + 1, cap (columns of a frame-store row), ctl_words (32-bit words of one sampling
 *             row), n_layer, Hkv, n_slots (rows of a kv head's cache), head_dim, esz (bytes of a cache element), im_end_id
 *   tok, tokn [max_batch][R]: the input column and the column under construction
 *   pos, nf, done [max_batch]
 *   seq [max_batch][R][cap]: the frame store
 *   ctl [max_batch][ctl_words]: the sampling rows (RowCtl) as raw words
 *   hid_in_xo [max_batch] bytes: the host's note of where ft_ar_get_debug(hidden) finds a slot's residual stream (1: the
 *             octet-major buffer of the MFMA launches).  This is the one piece of per-slot state that lives on the host.
 *   kv: the slow stack's caches, whole, [n_layer][K | V][max_batch][Hkv][n_slots][head_dim] in the cache's element type
 *             (ft_test_engine_handoffs reads one (layer, slot) per call; a byte check of every slot before and after every
 *             call wants them all at once). */
ft_status ft_test_ar_slots(ft_ctx* ctx, int32_t* geo, int32_t* tok, int32_t* tokn, int32_t* pos, int32_t* nf, int32_t* done,
                           int32_t* seq, uint32_t* ctl, uint8_t* hid_in_xo, void* kv);

/* Test hook (host code only: it synchronises the context's stream and copies device memory out; no kernel, no branch in a
 * kernel, nothing on the frame path): the hand-off vectors the frame engine's launches LEFT in device memory, decoded through
 * the kernels' own layout constants (frame_engine.h: ENG_LINE, EngLayout, the PK3 granules, VSTR, the y map of the slow
 * attention) into one (bf16 pattern, 16-bit tag) pair per unit.  Every hand-off buffer is double-buffered - the codebook
 * loop's by step parity with one buffer per layer, the slow stack's by layer parity - so after a launch the loop's last two
 * steps at every layer and the slow stack's last two layers are there.  A unit written by step / layer i of a launch that read
 * epoch word e carries the tag 0x8000 | ((e + i) & 0x7fff); every engine launch, slow or loop, advances the word by
 * epoch_step, so the last launch of a context read `epoch - epoch_step` (the slow launch of a whole frame: one more back).
 * which: 0 the slow stack, 1 the codebook loop.  copies (in): the copies of each vector the arrays have room for; (out) what
 * exists: 0 that engine is off, else 1 (copy 0: the source buffers) + 8 with the relay on (copy 1 + x: XCD x's replica).
 * Arrays (any may be NULL), uint16 values and tags, [copies][2 parities][layers][n]; parities the context did not allocate
 * (a one-layer slow stack) read as zeros, a tag no launch writes:
 *   which = 1: x [n_layer + 1][D] (entry n_layer: the stack's output), qkv [n_layer][QKVN], xb [n_layer][D], g [n_layer][F]
 *      read as plain granules, g3 [n_layer][F] read as PK3 triples (pk3 = 1 only; a triple shares its tag; which of the two
 *      forms a (step, layer) wrote is the kernel's: the paired first pass writes plain granules wherever position 0 goes on
 *      after the attention), log [1][V]; code: [copies][ncb][ENG_LINE] raw words of the code lines.
 *   which = 0: x, qkv, xb, g / g3 with layers = 1; y [1][HD]: unit i of the buffer at ymap(i) (the head-major order the
 *      Wo phase reads, for the split count of the last call); part [2][H][nsplit][hd + 2] f32 with part_tag (32-bit tags
 *      0x80000000 | (e + layer)): the split partials (O, then m, l), source only - they are not relayed.
 * K/V (kv_k and kv_v both non-NULL; works on a context whose engine is off as well): which = 0: rows [0, kv_rows) of slow
 * layer kv_layer of slot kv_slot, [Hkv][kv_rows][hd]; which = 1: the launch path's codebook-loop cache (fast_attn_kernel's
 * kc / vc) of fast layer kv_layer, [fast Hkv][kv_rows <= ncb][fast hd].  Bit patterns of the context's 16-bit type.
 * tab (which = 1, qkv0 = 1): row tab_row of the LOOP's own table of layer 0's q k v by drawn code (eng_qkv0_table_kernel;
 * ft_test_qkv0_tab reads the lock-step batches' table, another buffer built by another kernel), [QKVN] bf16 patterns.
 * In an f32 context kv_k / kv_v receive f32 values (twice the room; the pointers are declared for the 16-bit case).
 * FT_ERR_ARG: a bad which / layer / slot / row count; FT_ERR_STATE: a vector array on a context
 * whose engine of that kind is off, fewer copies than exist, a table row where there is no table. */
typedef struct ft_test_engine_io {
    int32_t which, copies;
    uint32_t epoch;
    int32_t epoch_step, n_layer, D, QKVN, HD, F, V, ncb, H, Hkv, hd;
    int32_t pk3, pair, qkv0, resident, relay, xl, nsplit, line;
    uint16_t *x, *x_tag, *qkv, *qkv_tag, *xb, *xb_tag, *g, *g_tag, *g3, *g3_tag, *log, *log_tag, *y, *y_tag;
    uint32_t* code;
    float* part;
    uint32_t* part_tag;
    int32_t kv_layer, kv_slot, kv_rows, tab_row;
    uint16_t *kv_k, *kv_v, *tab;
} ft_test_engine_io;
ft_status ft_test_engine_handoffs(ft_ctx* ctx, ft_test_engine_io* io);

/* Test hook: one draw of the sampling kernel (inference.py:30-80) on caller-supplied logits.
 * cb = 0 draws from `vocab_size` logits, cb >= 1 from min(1024, codebook_size); window is the
 * (num_codebooks+1) x 16 penalty window of inference.py:187-191 or NULL (no penalty); q the Exp(1)
 * noise (same length as the logits) or NULL (RNG).  Clobbers slot 0. */
ft_status ft_test_sample(ft_ctx* ctx, const float* logits, int32_t cb, const ft_sampling* sp,
                         const int32_t* window, const float* q, int32_t* out_index);

/* Test hook: ONE draw launch of M rows (1 <= M <= max_batch, rows 0 .. M - 1) through the product's own host routine
 * (engine.hip: enqueue_sample(L, cb, last)) on the context's own buffers, so the choice between sample_small_kernel, sample_block_kernel
 * and the four-launch draw, the lock-step form (wide_batch / wide_pair of an M-row launch) and the layer-0 q k v table are the
 * product's.  R = num_codebooks + 1, cap = max_new_tokens + 24, V = vocab_size (cb = 0) or min(1024, codebook_size).
 * In: logits [M][V]; sp [M]; noise [noise_rows][noise_row_len] in the layout ft_ar_set_noise takes (row = the drawing row's
 * nf, codebook cb at vocab_size + (cb - 1) fastV) or NULL (the counter-based generator).
 * In and out, whole, max_batch rows each (the caller puts sentinels wherever a draw must not write, rows M .. included):
 * tokn, tok [max_batch][R]; seq [max_batch][R][cap]; pos, nf, done [max_batch].
 * Out: logits_out [max_batch][V]: the M rows as the launch left them, then the 0xFF fill of rows M ..; femb [max_batch][fast_dim]; qkvf [2 ceil16(max_batch)][fast q k v width];
 * on a context with the lock-step path xo_femb and xo_x [dim / 8][xo_ldm][8] raw 16-bit (xo_ldm = 2 ceil16(max_batch)); cut
 * [max_batch][8] (the words of SampCut: kstar, nk, all_kept, argmax, Lmax, Mt, Z2, Tc), chunk_cnt, part_idx [max_batch x
 * ceil(vocab_size / 1024)], row m at m ceil(V / 1024).  All of these are filled with 0xFF bytes before the launch (a NaN in
 * every float type, -1 as an int), as are the logits rows M .., and the unused rows of the controls.
 * what: path (0 sample_small_kernel, 1 sample_block_kernel, 2 the four launches) | 4 the octet-major copy went to xo_femb | 8 to
 * rows xo_pair .. of xo_x (the paired pass) | 16 the q k v row came from the table.
 * Ends with every slot reset and the context's own noise back, also when a step of the hook fails.  FT_ERR_ARG: M, cb or last out of range, nf outside 0..cap or past the noise block, a noise row
 * shorter than vocab_size + (num_codebooks - 1) fastV, a missing argument. */
typedef struct ft_test_draw_io {
    int32_t M, cb, last, what;
    const float* logits;
    const ft_sampling* sp;
    const float* noise;
    int64_t noise_rows, noise_row_len;
    int32_t *tokn, *tok, *seq, *pos, *nf, *done;
    float *logits_out, *femb, *qkvf;
    uint16_t *xo_femb, *xo_x;
    int32_t *cut, *chunk_cnt, *part_idx;
} ft_test_draw_io;
ft_status ft_test_draw(ft_ctx* ctx, ft_test_draw_io* io);

/* Test hook: rows [row0, row0 + rows) of the table of fast layer 0's q k v by drawn code (lock-step batches) as raw 16-bit
 * patterns, [rows][fast q k v width]; *present = 0 and out untouched on a context that built none. */
ft_status ft_test_qkv0_tab(ft_ctx* ctx, int32_t row0, int32_t rows, uint16_t* out, int32_t* present);

/* Test hook: the resampler of ft_codec_decode_at on a host waveform x of n <= max_frames * frame_len samples at 44100
 * (zeros before and after it) -> y: *n_out = ft_resampled_len(sample_rate, n) samples. */
ft_status ft_test_resample(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, float* y, int64_t* n_out);

/* Test hook: the room stage's convolution launches alone (ft_codec_room; "Room") on taps the caller gives: c[i], i in [0, N),
 * is the stated chain over hn[0 .. L) and xs[0 .. n) with `predelay`.  1 <= n, N <= 2^28, 1 <= L <= 131072, 0 <= predelay
 * <= 48000; FT_ERR_ARG otherwise, before any device work. */
ft_status ft_test_room_conv(ft_ctx* ctx, const float* xs, int64_t n, const float* hn, int64_t L, int64_t predelay, int64_t N,
                            float* c);

/* Test hook: the time-scale stage of ft_codec_decode_fx alone on a host waveform x of n <= max_frames * frame_len samples
 * at 44100 -> y: *n_out = ft_timescaled_len(speed_pct, n) samples; deltas (may be NULL) receives the chosen d_k of the
 * *n_frames = ceil(*n_out / 512) + 1 frames. */
ft_status ft_test_timescale(ft_ctx* ctx, const float* x, int64_t n, int32_t speed_pct, float* y, int64_t* n_out,
                            int32_t* deltas, int32_t* n_frames);

/* Test hook: the time-scale and pitch stages of ft_codec_decode_fxp on a host waveform x of n <= max_frames * frame_len
 * samples at 44100 (cents != 0) -> y: *n_out = ft_timescaled_len(speed_pct, n) samples.  mid (may be NULL; room for 2 n + 1
 * samples) receives the *n_mid time-scaled samples the pitch stage read, deltas (may be NULL) the d_k of the *n_frames
 * frames of the time-scale stage at its rational rate.  With no time-scale stage *n_mid = n, mid = x and *n_frames = 0. */
ft_status ft_test_pitch(ft_ctx* ctx, const float* x, int64_t n, int32_t speed_pct, int32_t cents, float* y, int64_t* n_out,
                        float* mid, int64_t* n_mid, int32_t* deltas, int32_t* n_frames);

/* Test hook: the join stage of ft_codec_decode_join alone on B host waveforms, item b = x[b * stride .. b * stride + n[b])
 * (n[b] <= stride), which the hook uploads to the stage's input buffer as the decode leaves its items there.  y (room for
 * `capacity` >= sum(n) + sum(gaps) samples) receives the *total joined samples.  The hook fills the stage's output buffer
 * with the bit pattern 0xFFFFFFFE (a NaN) before the launches and copies all sum(n) + sum(gaps) samples of it back (the rest
 * of y, up to capacity, gets the same pattern on the host), so y[*total .. capacity) shows whether the stage wrote past its
 * output.  cuts: B x 2.  Refused
 * before any device work, y untouched: what ft_codec_decode_join refuses (FT_ERR_ARG), n[b] > stride (FT_ERR_ARG). */
ft_status ft_test_join(ft_ctx* ctx, const float* x, int32_t B, int64_t stride, const int64_t* n, const ft_join_params* jp,
                       const int64_t* gaps, int32_t started, float* y, int64_t capacity, int64_t* total, int64_t* cuts);

/* Test hook: the hop sums the level stage left in its last call on this context (ft_codec_loudness: one item; a joined call:
 * the items back to back), ceil(n / H) per item, the last one over what is left of the item.  *count = their number; the
 * first min(capacity, *count) go to hops. */
ft_status ft_test_level_hops(ft_ctx* ctx, double* hops, int64_t capacity, int64_t* count);

/* Test hook: a launch trace of the codec.  ft_test_codec_trace_arm makes the NEXT ft_codec_decode (B = 1; any other
 * B disarms it untraced), ft_codec_encode, ft_codec_stream_decode or ft_codec_stream_decode_many on this context
 * (ft_codec_stream_decode_many_at disarms it untraced) record one entry per kernel launch, in
 * launch order: a stable stage name ("post.2.wo", "up.1.pw1", "dec.3.u2.c7", "enc.2.sc", ...), the rows and columns
 * it wrote and, for a GEMM launch, the id of the instantiation picked (0 .. ft_test_codec_trace_variants() - 1, -1 for
 * the other kernels).  Launches [first, first + count) also keep a host copy of every buffer they wrote (bf16 as bf16,
 * f32 as f32, rows x cols dense), taken at that point of the stream because the work buffers are reused; the range
 * exists because a 215-frame trace held whole is several GB.  Recording only reads: the traced call's result equals
 * the untraced one bit for bit.  Off (one null-pointer test per launch) unless armed; the trace stays readable until
 * the next arm.
 * ft_test_codec_trace_count: launches the last traced call recorded (-1: a copy failed).
 * ft_test_codec_trace_variant: name and row / column tile of an instantiation id (NULL: no such id).
 * ft_test_codec_trace_launch: info[8] = {rows, cols, variant, buffers, halo rows, taps, K per tap, 1 if held}.
 * ft_test_codec_trace_buffer: buffer j of launch i: kind (0 out_bf / main output, 1 out_act (Snake'd copy), 2 out_f32),
 * is_f32, element count; dst != NULL receives the values (once: the copy is released).
 * A streamed call: the rows of a launch are the rows it wrote - one stream: the chunk's T x (rows per frame); the batched
 * call: the chunks' rows back to back in call order, the gap rows between them left out, so every buffer is dense
 * [sum L x rows per frame][cols].  A GEMM still reports the instantiation it ran (picked for the nominal utterance).
 * The carrying launches are recorded too, one entry per launch and chunk (chunks in call order), bf16, copied at that
 * point of the stream; info = {rows, cols, -1, buffers, rows, chunk index, 0, held}:
 *   "<stage>.roll" (tail_roll_kernel in front of <stage>: "up.0.dwln", "dec.in", "dec.1.ct", "dec.1.u2.c7", "final"):
 *       H x C; kind 3: the H rows in front of the chunk after the copy, kind 4: the whole carry left for the next chunk;
 *   "post.<l>.kvin" (kv_carry_in_kernel; only for a chunk with nh > 0): nh x 2 HD, kind 3: the K / V thirds of the nh
 *       rows placed in front of the chunk's q k v rows;
 *   "post.<l>.kvout" (kv_carry_out_kernel): (window - 1) x 2 HD, kind 4: the WHOLE carry left, rows the launch must not
 *       have written included.
 * ft_test_codec_trace_chunks: the chunk table of the last traced call: *n chunks (0: a one-shot call; 1: one stream),
 * table (may be NULL; room for 64 x 4) receives {P, L, t0, nh} per chunk: first frame in the call, frames, rope position,
 * carried K/V rows. */
ft_status ft_test_codec_trace_arm(ft_ctx* ctx, int32_t first, int32_t count);
int32_t ft_test_codec_trace_count(ft_ctx* ctx);
ft_status ft_test_codec_trace_chunks(ft_ctx* ctx, int32_t* n, int32_t* table);
int32_t ft_test_codec_trace_variants(void);
const char* ft_test_codec_trace_variant(int32_t id, int32_t* bm, int32_t* bn);
ft_status ft_test_codec_trace_launch(ft_ctx* ctx, int32_t i, char* name, int32_t cap, int32_t* info);
ft_status ft_test_codec_trace_buffer(ft_ctx* ctx, int32_t i, int32_t j, int32_t* kind, int32_t* is_f32, int64_t* elems,
                                     void* dst);

/* Test hook: a launch trace of the AR frame (host code only: no kernel, no branch in a kernel, nothing in a captured graph;
 * off, it costs one null-pointer test per launch site).  ft_test_ar_trace_arm makes the NEXT ft_ar_decode with n_frames == 1,
 * the NEXT ft_ar_first_frames or the NEXT prompt call (ft_ar_prefill_at / ft_ar_prefill, ft_ar_prefill_slow,
 * ft_ar_prefill_slow_many) on this context record one entry per kernel launch, in launch order; any other decode call disarms
 * it untraced.  The traced decode call launches its frame eagerly (the FT_NO_GRAPH branch), never from
 * a captured graph and never on the frame engine: arming a one-slot context whose frames run on the engine is FT_ERR_STATE,
 * and so is the armed call itself where it would go to the engine (one slot on a context that owns one; ft_ar_prefill_at on
 * any context that owns one, whose first frame's codebook loop runs there).
 * A prompt call (kinds 3, 4, 5).  prefill_gemm records "pf.embed", per layer "pf.<l>.norm1|wqkv|append|attn|wo|norm2|w13|w2",
 * "pf.last" (gather_last_rows_kernel, or the device-to-device copy of the last row into ctx->x) and, for kind 3, the tail under
 * the names of first frames ("fproj", "head", "draw.*", "fast.*").  cls[0]: a product's PF_ID_* (ft_test_pf_linear's *variant), the
 * append's 1 (prefill_rope_append_kernel) or 0, the attention's path (NG of the tiled kernel; 0: position by position).  m0 is the
 * slot of a single pass, 0 in a ragged one; rows the pass's rows.  A position-by-position prompt records the "embed" and
 * "slow.<l>.*" entries of each position k with "t<k>." in front, and the launch's pos_off (= pos0 + k; the device position is 0
 * after the reset).  A call of several passes - a ragged fill of more rows than max_seq_len, or ft_ar_prefill_slow_many falling back
 * to single passes, which is ONE trace over all of them - carries "pass<k>." in front of every name.  What the host uploaded for a
 * pass (d_prompt; pf_seqs and pf_rows in a ragged one) rides with the pass's first record.  State 0 and the record before the
 * first launch are taken BEFORE the call's ft_ar_reset, so the reset is part of what a reader judges; state 1 at the end of the call.
 * hid_in_xo of every slot a prompt call fills is 0 when the call returns (the single passes and the ragged pass alike: the slot's
 * hidden state is the row the pass left in ctx->x); read it with ft_test_ar_slots.
 * Recording only reads: the traced call's frames and the state it leaves equal the untraced call's bit for bit.
 * An entry: a stable name - "embed", "slow.<l>.wqkv|attn|wo|w13|w2" ("slow.<l>.attn.merge": attn_combine_rows_kernel behind a
 * split lock-step attention), "fproj", "xo_rows", "head", "draw.<cb>" (the four-launch draw: "draw.0.cut|count|race|finish"),
 * "fast.<cb>.<l>.wqkv|attn|wo|w13|w2" ("fast.pair.<l>...": codebook positions 0 and 1 in one pass), "fast.<cb>.head" -, the
 * row offset m0, the rows and the columns of the launch, and the class its dispatcher picked, cls[4]: a lock-step Linear
 * {WIDE_ID_*}; a gemv {MB, R, NT} ({-2, R, NT}: gemv_attn_combine_kernel); an attention {KV splits; 0: attn_wide_kernel}; a draw
 * launch {what} (ft_test_draw's word).  Entries [first, first + count) also keep a host copy of every buffer the launch wrote,
 * taken at that point of the stream and WHOLE: every row of the allocation, so the rows outside [m0, m0 + rows) can be held
 * against the record before.  Buffer ids (AR_TB_*), f32 [rows][cols] unless said: 0 x [max_batch][dim], 1 qkv, 2 y
 * [max_batch][y_ld], 3 g, 4 logits, 5 hid (x itself where fast_dim == dim), 6 femb, 7 xf, 8 qkvf [2 ceil16(max_batch)][fast q k v
 * width], 9 gf, 10 flog [max_batch][fastV], 11 part_o, 12 part_ml (flat: row m's partials at m H nsplit hd / m H nsplit 2 for
 * the call's split count); raw 16-bit octet-major [width / 8][xo_ldm][8], reported as rows = width / 8, cols = 8 xo_ldm: 20
 * xo_x, 21 xo_xf, 22 xo_femb, 23 xo_y, 24 xo_g; int32: 30 tokn, 31 tok [max_batch][R], 32 pos, 33 nf, 34 done [1][max_batch], 35
 * seq [max_batch][R cap], 36 cut [max_batch][8], 37 chunk_cnt, 38 part_idx [1][max_batch ceil(vocab / 1024)]; the prompt pass's
 * workspace, every one of its max_seq_len rows (prompt calls only, where the context has one): f32 13 pf_x [max_seq_len][dim], 14
 * pf_qkv, 15 pf_y [max_seq_len][H hd]; 16-bit ROW-major (rows, cols as said) 25 pf_xn [max_seq_len][dim], 26 pf_ybf, 27 pf_qbf
 * [max_seq_len][H hd], 28 pf_g [max_seq_len][intermediate]; int32 39 d_prompt [1][R max_seq_len], 40 pf_seqs [max_batch][4], 41 pf_rows
 * [max_seq_len][2].  A draw entry
 * lists every buffer finish_draw can write, written in this launch or not.  The K/V caches are not copied: read them before and
 * after the call with ft_test_engine_handoffs (which takes an f32 context too: its arrays then hold f32 values).
 * ft_test_ar_trace_count: launches the last traced call recorded (-1: a copy failed); info[5] (may be NULL) = {kind (0 none,
 * 1 a decode frame, 2 first frames, 3 ft_ar_prefill_at, 4 ft_ar_prefill_slow, 5 ft_ar_prefill_slow_many), m0 (kinds 3, 4: the slot; 5: 0),
 * rows of the call (kinds 3, 4: 1; 5: n), 1 if still armed, buffers of the record before the first launch}.
 * That record (launch index -1 of ft_test_ar_trace_buffer) holds every buffer listed above as the call found it: what a
 * buffer's first write in the call is held against.
 * ft_test_ar_trace_launch: info[10] = {m0, rows, cols, buffers, 1 if held, cls[0..3], pos_off}.
 * ft_test_ar_trace_buffer: info[4] = {id, bytes per element, rows, cols} of buffer j of launch i; dst != NULL receives it
 * (once: the copy is released).
 * ft_test_ar_trace_state: which = 0 before the first launch (after the call's controls went up and a frozen row's position was
 * put back inside its cache; a prompt call: before its reset), 1 at the end of the call: tok [max_batch][R], pos, nf, done [max_batch], seq [max_batch][R][cap]. */
ft_status ft_test_ar_trace_arm(ft_ctx* ctx, int32_t first, int32_t count);
int32_t ft_test_ar_trace_count(ft_ctx* ctx, int32_t* info);
ft_status ft_test_ar_trace_launch(ft_ctx* ctx, int32_t i, char* name, int32_t cap, int32_t* info);
ft_status ft_test_ar_trace_buffer(ft_ctx* ctx, int32_t i, int32_t j, int32_t* info, void* dst);
ft_status ft_test_ar_trace_state(ft_ctx* ctx, int32_t which, int32_t* tok, int32_t* pos, int32_t* nf, int32_t* done, int32_t* seq);

/* Test hook: ONE Linear of a lock-step batch through the product's own dispatcher (engine.hip: wide_gemm), so the tile
 * class, the K split and the choice of wide_head_kernel are the product's.  epi: 0 store (fused RMSNorm; f32 output
 * holding values of the model's type), 1 SwiGLU (fused RMSNorm; interleaved (gate, up) weight rows; N / 2 output columns),
 * 2 residual add (no norm).  X [M][K], W [N][K], gain [K] (epi 0 and 1), resid [M][N] (epi 2): bit patterns of the context's
 * 16-bit type; bias [N] f32 or NULL.  alias != 0 (epi 2): the output buffer IS the residual buffer (the product's
 * `xo, xo` form), otherwise they are two buffers (`xfo, xlo`).  The hook lays X and resid out octet-major at the context's
 * row stride xo_ldm = 2 x (max_batch rounded up to 16) with NaN patterns (0xFFFE) in operand rows M .. xo_ldm - 1, and
 * pre-fills the output with a sentinel (0xFFFE per 16-bit element, 0xFFFFFFFE per f32 element).  Everything lives in
 * temporaries of the call: no state of the context changes.
 * out: the M written rows, dense ([M][N] f32 for epi 0, else [M][N or N / 2] 16-bit patterns).  out_tail (room for 31
 * rows): the *tail_rows rows M .. 32 ceil(M / 32) - 1 of the output buffer, which must still hold the sentinel (in the
 * aliased form: the NaN fill of the residual rows).  *variant: the class that ran: 0 <1,1,norm,store>, 1 <1,2,norm,store>,
 * 2 <2,2,norm,store>, 3 <1,2,norm,SwiGLU>, 4 <2,2,norm,SwiGLU>, 5 <1,1,residual> (<batch tiles, weight tiles> of 16 rows
 * per workgroup; K picks the wave split), 6 wide_head_kernel.
 * FT_ERR_ARG for what the dispatcher would refuse: a model type that is not 16-bit, M outside 1..xo_ldm, K not in
 * {1024, 2048, 3072}, N not a whole number of the class's tiles. */
ft_status ft_test_wide_linear(ft_ctx* ctx, int32_t epi, int32_t vocab_head, int32_t M, int32_t N, int32_t K,
                              const uint16_t* X, const uint16_t* W, const uint16_t* gain, const float* bias,
                              const uint16_t* resid, int32_t alias, void* out, void* out_tail, int32_t* tail_rows,
                              int32_t* variant);

/* Test hook: the slow-stack attention launch of a lock-step batch of M <= min(max_batch, 64) rows at the context's head
 * geometry and rope table, through the product's own choice (engine.hip: wide_attn) between attn_wide_kernel<Gq> and
 * attn_decode_kernel + attn_combine_rows_kernel.  qkv [M][(H + 2 Hkv) hd] f32, pos [M] (the new position of each row:
 * its context is pos + 1 long), qn / kn [hd] and the caches kc / vc [M][Hkv][n_slots][hd] as 16-bit patterns.  The hook
 * works on temporaries (only the context's split-partial scratch is written): kc / vc are uploaded, the launch appends
 * row pos[m], and both come back whole in place, so a caller can see every other row unchanged.  y [M][H hd]: 16-bit
 * patterns read back from the octet-major operand buffer.  *splits: 0 = attn_wide_kernel ran, n >= 1 = the fall-back
 * with n KV splits (n > 1: merged by attn_combine_rows_kernel). */
ft_status ft_test_wide_attn(ft_ctx* ctx, int32_t M, const float* qkv, const int32_t* pos, const uint16_t* qn,
                            const uint16_t* kn, uint16_t* kc, uint16_t* vc, uint16_t* y, int32_t* splits);

/* Test hook: ONE Linear product of the bf16 prompt pass through the product's own dispatcher (engine.hip: pf_gemm), unchanged,
 * so the choice between skinny_gemm_kernel<TS>, lingemm_kernel<128,128>, lingemm_kernel<64,64>, the two tapgemm64_kernel tiles
 * and the tapgemm_kernel fall-backs is the product's (FT_PREFILL_GEMM, read when the context is created, is honoured).  form
 * picks one of the four calls prefill_gemm makes: 0 wqkv (f32 store of bf16-rounded values), 1 wo / w2 (f32 residual added to
 * the rounded product, the sum rounded; alias != 0: the output buffer IS the residual buffer, as the product runs it, otherwise
 * two buffers), 2 w13 (SwiGLU on interleaved (gate, up) weight rows, N / 2 bf16 output columns).  X [S][K], W [N][K]: bf16
 * patterns; bias [N] f32 or NULL; resid [S][N] f32 (form 1).  The hook allocates X and the output with 128 ceil(S / 128) rows:
 * X rows from S on hold NaN patterns (0xFFFE), output (and residual) rows from S on the sentinel (0xFFFE per 16-bit element,
 * 0xFFFFFFFE per f32 element).  Everything lives in temporaries of the call: no state of the context changes.
 * out: the S written rows, dense ([S][N] f32 for forms 0 and 1, [S][N / 2] bf16 patterns for form 2).  out_tail (room for 127
 * rows): the *tail_rows rows S .. 128 ceil(S / 128) - 1 of the output buffer - past the row-tile edge of every class - which
 * must still hold the sentinel.  *variant: the kernel class that ran: 0 / 1 / 2 skinny_gemm_kernel<1 / 2 / 4>, 3
 * lingemm_kernel<128,128>, 4 lingemm_kernel<64,64>, 5 tapgemm64_kernel<128,128>, 6 tapgemm64_kernel<64,64>, 7
 * tapgemm_kernel<128,128>, 8 tapgemm_kernel<128,64>.
 * The fused-norm arguments of pf_gemm (PfX: gain, ss_in, ss_out) have no caller in the prompt pass and none here.
 * FT_ERR_ARG: a context that is not bf16, S outside 1..max_seq_len, K not a multiple of 32, N not a multiple of 16, a missing
 * argument; FT_ERR_STATE: a context whose prompts run position by position (FT_PREFILL_V0, widths off the MFMA tiles). */
ft_status ft_test_pf_linear(ft_ctx* ctx, int32_t form, int32_t S, int32_t N, int32_t K, const uint16_t* X, const uint16_t* W,
                            const float* bias, const float* resid, int32_t alias, void* out, void* out_tail,
                            int32_t* tail_rows, int32_t* variant);

/* Test hook: rmsnorm_llama_rows_kernel<bf16, round> of the prompt pass on S f32 rows x [S][D] with gain [D] (bf16 patterns)
 * at the context's norm_eps -> out [S][D] bf16 patterns; out_tail [D]: the row behind them, which must still hold 0xFFFE.
 * Refusals as ft_test_pf_linear. */
ft_status ft_test_pf_norm(ft_ctx* ctx, int32_t S, int32_t D, const float* x, const uint16_t* gain, uint16_t* out,
                          uint16_t* out_tail);

/* Test hook: the attention of ONE layer of a prompt pass at the context's head geometry and rope table - the K/V append of
 * every row, then the causal attention - through the host routine prefill_gemm itself calls (engine.hip: pf_attn), so the
 * choice between flash_prefill_kernel<HD, NG> (NG = 4 up to 320 grid rows, else 2) and attn_decode_kernel position by position
 * (fewer than 16 rows, FT_PREFILL_ATTN_V0) is the product's.  n_seq = 0: one prompt of Lp rows at cache positions
 * pos0 .. pos0 + Lp - 1 of `slot`.  n_seq >= 1: the ragged pass, seqs [n_seq][4] = {first row, rows, first cache position,
 * slot}, rows back to back, slots distinct (Lp, pos0, slot ignored).  qkv [S][(H + 2 Hkv) hd] f32 (S = all rows), qn / kn [hd]
 * and the caches kc / vc [max_batch][Hkv][n_slots][hd] as bf16 patterns.  The hook writes NaN patterns (0xFFFE) into every
 * cache row at or behind a sequence's pos0 + rows and into every slot no sequence names, uploads both caches, runs the pass on
 * temporaries and returns them whole in place.  y, q [S][H hd]: the attention output and the finished (normalised, rotated)
 * queries as bf16 patterns - q stays 0xFFFE on the per-position path, which keeps its queries in LDS.  tail [2][H hd]: the row
 * behind y and behind q (0xFFFE).  *path: NG of the tiled kernel, 0 = position by position.
 * FT_ERR_ARG for what the product would refuse (a bad or repeated slot, an empty prompt, pos0 + rows >= max_seq_len, more rows
 * than max_seq_len, a ragged pass where the tiled kernel does not run) and a context that is not bf16; FT_ERR_STATE as above. */
ft_status ft_test_pf_attn(ft_ctx* ctx, int32_t n_seq, const int32_t* seqs, int32_t Lp, int32_t pos0, int32_t slot,
                          const float* qkv, const uint16_t* qn, const uint16_t* kn, uint16_t* kc, uint16_t* vc, uint16_t* y,
                          uint16_t* q, uint16_t* tail, int32_t* path);

/* Test hook: ONE product of a decode launch of M in 1..max_batch rows through the product's own dispatcher (engine.hip: gemv), with
 * R = rows_per_wave(N, M) as every caller passes it, so the choice between gemv_kernel<NT, R> and gemv_mb_kernel<NT, R, MB> is
 * the product's.  pro: 0 none, 1 fused RMSNorm (gain [K]); epi: 0 store, 1 residual add, 2 SwiGLU on interleaved (gate, up)
 * weight rows (N / 2 output columns).  x [M][K] f32 (dense: the hook lays it out at row stride ldx >= K); W [N][K], gain [K]
 * and bias [N] (or NULL) in the context's type - bit patterns of the 16-bit type, f32 in an f32 context; resid [M][N] f32 (epi
 * 1).  alias != 0 (epi 1): the output buffer IS the residual buffer, as the slow layers run it (`x, x`), otherwise two
 * buffers, as fast layer 0 runs it.  nt: non-temporal weight loads.  ldx, ldo: multiples of 4, ldo >= the output columns.
 * x is allocated with 4 ceil(M / 4) rows: the hook fills rows M .. and the ldx padding with NaN patterns, and the output - [M + 1][ldo], the residual buffer in
 * the aliased form - with 0xFFFFFFFE before the launch.  Everything lives in temporaries of the call.
 * out [M + 1][ldo]: the whole output buffer: the written rows, their padding columns and the row behind row M - 1, which
 * must still hold the sentinel.  id[3] = {MB (0: gemv_kernel), R, NT} of the launch.
 * FT_ERR_ARG: what gemv refuses (K above 12 x 64 16-byte pieces), K not a multiple of 8, M outside 1..max_batch, an odd N for SwiGLU,
 * a bad stride, a missing argument. */
ft_status ft_test_gemv(ft_ctx* ctx, int32_t pro, int32_t epi, int32_t M, int32_t N, int32_t K, const float* x, int32_t ldx,
                       const void* W, const void* gain, const void* bias, const float* resid, int32_t alias, int32_t nt,
                       int32_t ldo, float* out, int32_t* id);

/* Test hook: the "decode attention, then Wo" part of a slow layer for M in 1..max_batch rows at the context's head geometry and rope
 * table, through the host routine enqueue_slow itself calls (engine.hip: decode_attn_wo): attn_decode_kernel over the
 * context's KV splits, then gemv_attn_combine_kernel (more than one split: the merge of the partials rides inside the Wo
 * product) or the plain product.  The split count is picked first, as ft_ar_decode picks it, for a call whose longest context
 * ends at max(pos) + pos_off + 1, and the context's own value is put back afterwards.  qkv [M][(H + 2 Hkv) hd] f32, pos [M]
 * (the device position; pos + pos_off is the appended row), qn / kn [hd] or NULL, the caches kc / vc [M][Hkv][n_slots][hd],
 * wo [dim][H hd] and bo [dim] or NULL in the context's type (patterns; f32 in an f32 context), resid [M][dim] f32.
 * Temporaries of the call but for the context's split-partial scratch (row m's partials at m H nsplit hd, as decode_attn_wo
 * places them; its room is max_batch rows).  Outputs: *nsplit; y [M][y_ld] (y_ld = max(H hd,
 * fast H x hd)): with one split the attention output, otherwise still the 0xFFFFFFFE fill; with more than one split
 * part_o [M][H][nsplit][hd] and part_ml [M][H][nsplit][2] as the kernel left them (pre-filled with the sentinel); x_out
 * [M][dim]: the residual stream after the Wo product (in place, as the product runs it); kc / vc back whole in place.
 * part_o / part_ml need room for 32 splits.  FT_ERR_ARG: M outside 1..max_batch, a position outside the cache or the
 * rope table, a missing argument. */
ft_status ft_test_decode_attn(ft_ctx* ctx, int32_t M, const float* qkv, const int32_t* pos, int32_t pos_off, const void* qn,
                              const void* kn, void* kc, void* vc, const void* wo, const void* bo, const float* resid,
                              int32_t* nsplit, float* y, float* part_o, float* part_ml, float* x_out);

/* Test hook: one embed_kernel launch (grid ((D + 255) / 256, M)) on caller tables; the sizes are the call's, not the
 * context's, only the element type is.  emb [vocab][D], cb_emb [ncb x cbsize][D] in the context's type; toks: n_toks ints,
 * row m's token at toks[m tok_m_stride], its code i at toks[m tok_m_stride + (i + 1) tok_row_stride].  x [M + 1][ldx] f32: the
 * whole buffer, pre-filled with 0xFFFFFFFE (padding columns and the row behind row M - 1 must keep it).  xo_ldm > 0 (16-bit
 * contexts): xo [ceil(D / 8)][xo_ldm][8], the octet-major 16-bit copy, pre-filled with 0xFFFE (rows M .. xo_ldm - 1 keep it).
 * FT_ERR_ARG: a bad size, strides that reach past n_toks, M > xo_ldm, an octet-major copy in an f32 context. */
ft_status ft_test_embed(ft_ctx* ctx, int32_t M, int32_t D, int32_t ncb, int32_t cbsize, int32_t vocab, const void* emb,
                        const void* cb_emb, const int32_t* toks, int64_t n_toks, int64_t tok_row_stride, int64_t tok_m_stride,
                        int32_t sem_begin, int32_t sem_end, int32_t scale, int32_t ldx, int32_t xo_ldm, float* x, uint16_t* xo);

/* Test hook: ONE fast_attn_kernel launch at the context's fast-stack geometry and its `frope` table, in one of three forms.
 * form 0, single: M in 1..max_batch rows at codebook position c in 0..ncb-1, y [M + 1][y_ld] f32 (the whole buffer, pre-filled with
 * 0xFFFFFFFE: padding columns and the row behind row M - 1 keep it).  form 1, wide single: M in 5..64, y_bf [H hd / 8][xo_ldm][8]
 * 16-bit patterns, octet-major at the context's xo_ldm, pre-filled with 0xFFFE.  form 2, paired: pair_M = M; qkv rows [0, M)
 * are the utterances at position 0, qkv rows [M, 2 M) the same utterances at position 1 (the hook places them at rows
 * xo_pair .. xo_pair + M - 1, NaN patterns between), grid 2 M, c ignored; y_bf as form 1 (rows [0, M) and [xo_pair, xo_pair + M)).
 * qkv [rows][(H + 2 Hkv) hd] f32; qn / kn [hd] or NULL and the caches kc / vc [M][Hkv][ncb][hd] in the context's type.  The hook
 * writes NaN patterns into cache rows c .. ncb - 1 (paired: 0 .. ncb - 1) in place, uploads, launches on temporaries and
 * returns both caches whole in place.
 * The paired form is wider than the product's rule (wide_pair: xo_pair + M <= 64) on purpose: on a context of up to 64 rows it
 * takes every M up to xo_ldm - xo_pair, so that one 64-row context serves every tile edge; on a context above 64 rows, where
 * the product pairs at no M, it is refused.
 * FT_ERR_ARG: a bad form, M or c, a missing argument, a wide form in an f32 context, a paired pass past xo_ldm or on a context
 * above 64 rows (xo_pair > 64);
 * FT_ERR_STATE: a wide form on a context without the lock-step MFMA path. */
ft_status ft_test_fast_attn(ft_ctx* ctx, int32_t form, int32_t M, int32_t c, const float* qkv, const void* qn, const void* kn,
                            void* kc, void* vc, float* y, uint16_t* y_bf);

/* Test hook: the ride stage alone (fishtts_hip.h: "Ride") on B host waveforms run as B carried streams in the same calls.
 * x [B][stride], waveform b has n[b] <= stride samples at sample_rate; target as ft_codec_ride's, not 0.  There are
 * ncuts + 1 calls: call j gives every stream its samples in [cuts[j-1], cuts[j]) (cuts[-1] = 0, cuts non-descending), clipped
 * to n[b]; the last call takes what is left and is `final`.  y [B][stride] receives each stream's emitted samples one call
 * after the other, nodes [B][stride / H + 2] its ceil(n[b] / H) + 1 nodes, emitted[j B + b] what call j gave stream b. */
ft_status ft_test_ride_streams(ft_ctx* ctx, const float* x, int32_t B, int64_t stride, const int64_t* n, int32_t sample_rate,
                               int32_t target, const int64_t* cuts, int32_t ncuts, float* y, float* nodes, int64_t* emitted);

#ifdef __cplusplus
}
#endif
#endif
