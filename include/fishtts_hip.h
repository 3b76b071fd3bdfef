/* libfishtts_hip.so — C ABI of the MI355X (gfx950) hot path: dual-AR semantic-token decode +
 * DAC codec decode (and encode, for encode_reference).  Plain pointers and sizes only; no torch types.
 *
 * The reference (smolGura/fish-tts) is pure Python and has no FFI; the seams this library
 * sits behind are the Python-level operators named in SURVEY.md §8(b).  Each entry point
 * cites the reference interface it replaces (paths relative to /root/reference).
 *
 * Threading: AR calls on one ctx are serialized by the caller (as the reference's
 * synthesize() is not re-entrant: synthesizer.py:431-481 shares one KV cache);
 * ft_codec_decode is re-entrant with respect to AR calls and runs on its own HIP stream
 * (mirrors the decoder thread of synthesizer.py:513-528).  One ctx per GPU.
 *
 * Ownership: the caller owns every buffer it passes; the library copies weights into its
 * own HBM allocations and never frees caller memory.  Errors: integer status + a message
 * from ft_last_error(); the Python host maps them to the reference's ValueError/RuntimeError.
 */
#ifndef FISHTTS_HIP_H
#define FISHTTS_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ft_ctx ft_ctx;
typedef int32_t ft_status;

enum { FT_OK = 0, FT_ERR_ARG = 1, FT_ERR_HIP = 2, FT_ERR_STATE = 3, FT_ERR_UNSUPPORTED = 4,
       FT_ERR_NOMEM = 5, FT_ERR_TOO_LONG = 6, FT_ERR_MISSING_WEIGHT = 7 };
enum { FT_F32 = 0, FT_BF16 = 1, FT_F16 = 2 };   /* FT_F16: the AR model only (precision="fp16", synthesizer.py:125-126) */

/* Field names and meaning = config.json / DualARModelArgs (fish_tts/models/llama.py:31-123);
 * the three token ids come from the tokenizer layout (fish_tts/models/tokenizer.py:83-101). */
typedef struct ft_ar_config {
    int32_t dtype;  /* FT_BF16 | FT_F16 | FT_F32: model precision (fish_tts/synthesizer.py:122-128) */
    int32_t vocab_size, n_layer, n_head, dim, intermediate_size, n_local_heads, head_dim;
    float rope_base, norm_eps;
    int32_t max_seq_len, tie_word_embeddings, attention_qkv_bias, attention_o_bias, attention_qk_norm;
    int32_t codebook_size, num_codebooks, scale_codebook_embeddings;
    int32_t n_fast_layer, fast_dim, fast_n_head, fast_n_local_heads, fast_head_dim,
        fast_intermediate_size, fast_attention_qkv_bias, fast_attention_qk_norm, fast_attention_o_bias;
    int32_t semantic_begin_id, semantic_end_id, im_end_id;
    int32_t max_batch;      /* utterance slots decoded in lock step (reference: 1, inference.py:313-317) */
    int32_t max_new_tokens; /* per-slot capacity for generated frames */
} ft_ar_config;

/* Hyper-parameters of the DAC decode path; the reference hard-codes them in
 * fish_tts/synthesizer.py:199-269 (and fish_tts/models/vocoder.py:824-872). */
typedef struct ft_codec_config {
    int32_t dtype;                 /* FT_BF16 only: bf16 MFMA contractions, f32 accumulation, f32 transformer residual stream (anything else is FT_ERR_UNSUPPORTED) */
    int32_t n_codebooks;           /* residual codebooks (9); +1 semantic */
    int32_t codebook_size, semantic_codebook_size, codebook_dim, latent_dim; /* 1024, 4096, 8, 1024 */
    int32_t n_tf_layer, tf_n_head, tf_head_dim, tf_ffn, tf_window;           /* 8, 16, 64, 3072, 128 */
    float tf_rope_base, tf_norm_eps;                                          /* 1e4, 1e-5 */
    int32_t n_upsample;            /* 2 (x2 each) */
    int32_t decoder_dim;           /* 1536 */
    int32_t n_rates;               /* 4 */
    int32_t rates[8];              /* 8,8,4,2 */
    int32_t max_frames;            /* longest code sequence per call */
    int32_t max_batch;
    /* encode side (encode_reference: synthesizer.py:325-357, Encoder vocoder.py:498-575); encoder_dim = 0: decode only */
    int32_t encoder_dim;           /* 64 */
    int32_t n_enc_rates;           /* 4 */
    int32_t enc_rates[8];          /* 2,4,8,8 */
    int32_t enc_tf_layers[8];      /* 0,0,0,4: window-limited transformer layers after each block's strided conv */
    int32_t enc_tf_window;         /* 512 */
    int32_t max_enc_frames;        /* longest reference in code frames (a frame = prod(enc_rates)*4 samples) */
} ft_codec_config;

/* Sampling scalars of synthesize()/generate_long() (synthesizer.py:431-439, inference.py:741-765). */
typedef struct ft_sampling {
    float temperature, top_p, repetition_penalty;
    int32_t ban_eos;   /* 1: mask <|im_end|> before sampling (fixed-length synthetic benches only) */
    uint64_t seed;     /* counter-based RNG stream for the Exp(1) race (inference.py:24-27) */
} ft_sampling;

/* Lifecycle.  Replaces init_model() + setup_caches() (inference.py:387-414, llama.py:378-398,544-559)
 * and _load_vocoder() (synthesizer.py:188-293).  Either config may be NULL. */
ft_status ft_create(const ft_ar_config* ar, const ft_codec_config* codec, int32_t device, ft_ctx** out);
void ft_destroy(ft_ctx* ctx);
const char* ft_last_error(const ft_ctx* ctx); /* ctx may be NULL: last create-time error */

/* Weight ingestion under the reference's state-dict names (llama.py:349-359,510-535 after the
 * wq/wk/wv->wqkv fuse of llama.py:222-227; codec names as vocoder.py modules after weight-norm
 * folding).  `src` may be a host or a device pointer; `src_dtype` FT_F32|FT_BF16|FT_F16; the tensor is
 * converted to the ctx precision and repacked.  Replaces load_state_dict (llama.py:498). */
ft_status ft_load_weight(ft_ctx* ctx, const char* name, const void* src, int32_t src_dtype,
                         const int64_t* shape, int32_t ndim);
ft_status ft_finalize_weights(ft_ctx* ctx); /* checks completeness, builds fused layouts + tables */

/* AR path.  A "slot" is one utterance's state (KV cache, position, penalty window, RNG). */
ft_status ft_ar_reset(ft_ctx* ctx, int32_t slot);
/* Prefill = the un-compiled first decode_one_token_ar call of generate()/generate_streaming()
 * (inference.py:353-362, 709-718): prompt is (num_codebooks+1) x Lp int32 row-major, host memory
 * (ContentSequence.encode_for_inference output, inference.py:611-640).  Writes the first
 * generated frame (num_codebooks+1 int32) to out_frame (host).  No repetition penalty. */
ft_status ft_ar_prefill(ft_ctx* ctx, int32_t slot, const int32_t* prompt, int32_t Lp,
                        const ft_sampling* sp, int32_t* out_frame);
/* Several prompts at once (a batch scheduler's initial fill): ft_ar_prefill_slow runs the prompt pass of one slot
 * without its first frame (K/V + last hidden state stay on the device); ft_ar_first_frames then draws the first frames
 * of the contiguous slots [slot0, slot0+n) in one lock-step pass (head, semantic draw, fast codebooks) - the per-slot
 * equivalent is ft_ar_prefill_at.  next_pos[i] = pos0_i + Lp_i; out_frames: n x (num_codebooks+1) int32 (host). */
ft_status ft_ar_prefill_slow(ft_ctx* ctx, int32_t slot, const int32_t* prompt, int32_t Lp, int32_t pos0);
ft_status ft_ar_first_frames(ft_ctx* ctx, int32_t slot0, int32_t n, const ft_sampling* sp, const int32_t* next_pos,
                             int32_t* out_frames);
/* Prompt passes of n distinct slots in one call (a batch scheduler's initial fill and refills; the reference runs one
 * prompt pass per utterance, inference.py:353-362).  prompts: the n matrices back to back, matrix i = (num_codebooks+1) x
 * Lps[i] int32 row-major; slot i's prompt lands at cache positions [pos0s[i], pos0s[i] + Lps[i]).  From the width at
 * which lock-step batches run on the MFMA launches (5 prompts, bf16) all prompts go through the slow stack as the rows
 * of ONE pass (weights streamed once; K/V append and attention by sequence) - results follow the oracle within the bf16
 * evaluation-order margin, like the lock-step frames of that width; below it (and in fp16 / fp32) the call equals n calls
 * of ft_ar_prefill_slow bit for bit.  Follow with ft_ar_first_frames per contiguous run of slots. */
ft_status ft_ar_prefill_slow_many(ft_ctx* ctx, int32_t n, const int32_t* slots, const int32_t* prompts,
                                  const int32_t* Lps, const int32_t* pos0s);
/* Marks a slot idle for lock-step decoding: it counts as already finished (ft_ar_decode reports 0 frames for
 * it and it limits nothing); a later ft_ar_prefill[_at] on the slot re-activates it.  Slots that emit
 * <|im_end|> freeze the same way on the device, so a host scheduler can refill finished slots between
 * ft_ar_decode bursts (continuous batching; the reference serves one utterance at a time, synthesizer.py:431). */
ft_status ft_ar_park(ft_ctx* ctx, int32_t slot);
/* Moves the live utterance of slot `from` to slot `to` between ft_ar_decode calls (a continuous-batching scheduler keeps
 * its active slots at [0, n) so that a lock-step step of width n - and a lone survivor on slot 0, the batch-1 frame
 * engine - serves them; the reference serves one utterance at a time, synthesizer.py:431).  Carried: the slow stack's K/V
 * rows [0, pos) of every layer, the slot's row of the frame store (the repetition-penalty window reads it), position,
 * input column, frame count, done flag and sampling row; `from` is left parked (as ft_ar_park leaves it), `to`'s former
 * content is overwritten.  One launch, stream-ordered after every earlier call.  Refused before any device work, both
 * slots unchanged: FT_ERR_ARG (a slot out of range, from == to), FT_ERR_STATE (a context without the AR model).
 * Not carried: the residual stream of the slot's last frame.  ft_ar_get_debug(hidden) of `to` is defined only after its
 * next frame (the logits row is not carried either); K/V rows >= pos of `to`, every other slot and the K/V, column under
 * construction and sampling row of `from` stay as they are. */
ft_status ft_ar_slot_move(ft_ctx* ctx, int32_t from, int32_t to);
/* Reference-prefix KV reuse (the reference keeps the reference tensors in
 * `_prefill_cache` but re-prefills them on every call: synthesizer.py:363-429, inference.py:779-793,
 * 353-362).  The prompt prefix [<|interleave|>, (<|speaker:0|>, ref text, ref codes, <|im_end|>)*] does
 * not depend on the text to speak, and the model is causal, so its K/V are computed once:
 *   ft_ar_prefill(slot, prefix)  ->  ft_ar_kv_save(slot, n_prefix)            (once per voice)
 *   ft_ar_kv_restore(snap, slot) ->  ft_ar_prefill_at(slot, tail, pos0=n_prefix)  (per utterance)
 * ft_ar_prefill_at feeds `Lp` prompt columns at cache positions [pos0, pos0+Lp) of a slot whose
 * positions [0, pos0) already hold K/V; pos0 = 0 is ft_ar_prefill. */
typedef struct ft_kv_snapshot ft_kv_snapshot;
ft_status ft_ar_prefill_at(ft_ctx* ctx, int32_t slot, const int32_t* prompt, int32_t Lp, int32_t pos0,
                           const ft_sampling* sp, int32_t* out_frame);
ft_status ft_ar_kv_save(ft_ctx* ctx, int32_t slot, int32_t n_pos, ft_kv_snapshot** out);
ft_status ft_ar_kv_restore(ft_ctx* ctx, const ft_kv_snapshot* snap, int32_t slot);
int32_t ft_ar_kv_positions(const ft_kv_snapshot* snap);
void ft_ar_kv_free(ft_ctx* ctx, ft_kv_snapshot* snap);
/* Decode loop = decode_n_tokens[_streaming] (inference.py:158-276) driving decode_one_token_ar
 * (inference.py:83-155), for slots [0, nslots) in lock step, up to n_frames more frames each.
 * out_frames: nslots x n_frames x (num_codebooks+1) int32 (host), frame-major; out_n[slot] =
 * frames produced (the <|im_end|> frame included, as the streaming loop yields it).
 * The step is hipGraph-captured; EOS is polled every `poll` frames (>=1).
 * A call runs no live slot past position max_seq_len - 1 (the last row of the rope table; the cache has max_seq_len rounded
 * up to 8 rows) nor past its frame store.  A slot that finished on its last cache row may stay in the batch until the
 * caller parks or refills it: frozen, it rewrites that row of its own cache and nothing else. */
ft_status ft_ar_decode(ft_ctx* ctx, int32_t nslots, int32_t n_frames, const ft_sampling* sp,
                       int32_t poll, int32_t* out_frames, int32_t* out_n);

/* Codec path = DAC.decode (vocoder.py:906-912) incl. DownsampleResidualVectorQuantize.decode
 * (vocoder.py:800-814) and Decoder (vocoder.py:605-640).  codes: B x (n_codebooks+1) x T int32
 * (host), right-padded; lens[b] valid frames.  audio: B x (T*frame_len) float32 (host),
 * samples beyond lens[b]*frame_len are written but meaningless (the codec is causal). */
ft_status ft_codec_decode(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                          float* audio);
int32_t ft_codec_frame_len(const ft_ctx* ctx); /* samples per code frame (2048) */
/* Streamed decode with carried state (second half).  The reference's synthesize_stream decodes
 * every chunk from zero state (synthesizer.py:513-528, 591-595); the codec is strictly causal (window-128 attention,
 * vocoder.py:325-332; left-padded convolutions, vocoder.py:411-420, 449-455), so carrying the last 127 frames' K/V of
 * every transformer layer and the last `halo` rows of every convolution input makes the chunks of one stream
 * concatenate to exactly the waveform of one decode of all the codes.  codes: (n_codebooks+1) x T int32 (host), audio:
 * T * frame_len float32 (host).  A stream holds at most max_frames frames.  Kernel variants are chosen as for a 215-frame
 * utterance whatever the chunk length, so the result does not depend on the chunking. */
typedef struct ft_codec_stream ft_codec_stream;
ft_status ft_codec_stream_begin(ft_ctx* ctx, ft_codec_stream** out);
ft_status ft_codec_stream_decode(ft_ctx* ctx, ft_codec_stream* st, const int32_t* codes, int32_t T, float* audio);
void ft_codec_stream_end(ft_ctx* ctx, ft_codec_stream* st);
/* One chunk of each of n distinct streams of this context, in ONE pass through the codec (the kernels take the chunk from
 * the grid's z dimension: the launches do not depend on n).  codes: n blocks back to back, block j = (n_codebooks+1) x
 * lens[j] int32 row-major (host); audio: lens[j] * frame_len float32 per stream, back to back (host).  Stream j's samples
 * and carried state are, bit for bit, those ft_codec_stream_decode gives for the same chunk; streams may stand at
 * different positions and chunks differ in length.  Limits: 1 <= n <= 64, lens[j] >= 1, sum(lens) <= max_frames,
 * t0 + lens[j] <= max_frames.  Every argument is checked before any device work; a refused call changes no stream:
 * FT_ERR_ARG (bad n, lens[j] < 1, a null pointer, a stream named twice), FT_ERR_STATE (a stream of another or a destroyed
 * context), FT_ERR_TOO_LONG (n > 64, a stream past max_frames, sum(lens) > max_frames).  The first call allocates the
 * batch workspace: 4 conv buffers of (max_frames x the widest per-frame row + 63 x 64 rows of max(4 latent_dim,
 * decoder_dim)) bf16 each, a q k v buffer of (max_frames + 64 (tf_window - 1)) x 3 n_head head_dim bf16 and a table of
 * chunks, carry pointers and codes (< 1 MB); it lives as long as the context. */
ft_status ft_codec_stream_decode_many(ft_ctx* ctx, int32_t n, ft_codec_stream* const* streams, const int32_t* codes,
                                      const int32_t* lens, float* audio);
/* Resampled output.  The codec runs at Fi = 44100 Hz; these calls give its waveform at a caller-chosen rate Fo through a
 * polyphase FIR resampler on the device (Fo / Fi reduced to L / M; output n is the value at input time n M / L, the
 * filter's delay compensated).  Weights: a Kaiser-windowed sinc, pass band to 0.43 min(Fi, Fo) (<= 0.01 dB ripple), stop
 * band from 0.5 min(Fi, Fo) (>= 70 dB), designed once per rate on the host in float64 and kept as float32 [L][K] (phase p,
 * tap t: output n with n M = i0 L + p sums w[p][t] x[i0 - K/2 + 1 + t] over t = 0 .. K-1 in that order, in float32).
 * Accepted rates: integers in [8000, 48000] whose L is at most 640 (8000, 11025, 12000, 16000, 22050, 24000, 32000,
 * 48000 among them); 44100 takes the codec's own path and runs no resampler.  Anything else is FT_ERR_ARG before any
 * device work.  The reference returns 44.1 kHz only (synthesizer.py:431-481). */
/* Host only (no context, no device): validates the rate; L, M, K (K = 0 at 44100) and, if `table` is non-null, the
 * L x K weights.  Any output pointer may be NULL. */
ft_status ft_resample_filter(int32_t sample_rate, int32_t* L, int32_t* M, int32_t* K, float* table);
/* ceil(n_in L / M) - the samples n_in codec samples give at sample_rate; -1 for a refused rate. */
int64_t ft_resampled_len(int32_t sample_rate, int64_t n_in);
/* ft_codec_decode at sample_rate: utterance b yields out_lens[b] = ft_resampled_len(sample_rate, lens[b] * frame_len)
 * samples (zeros before and after it), zero-padded past its end; audio: B x max(out_lens) float32 (host). */
ft_status ft_codec_decode_at(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                             int32_t sample_rate, float* audio, int64_t* out_lens);
/* A streamed decode whose output is at sample_rate (44100: ft_codec_stream_begin).  Besides the codec's carries, such a
 * stream keeps the last K input samples (two copies: a call reads one and writes the other) and its input / output
 * sample counters.  ft_codec_stream_decode and ft_codec_stream_decode_many refuse it (FT_ERR_STATE). */
ft_status ft_codec_stream_begin_at(ft_ctx* ctx, int32_t sample_rate, ft_codec_stream** out);
/* ft_codec_stream_decode_many for streams of any rate, mixed in one call.  A chunk emits the outputs whose taps all lie
 * within the input seen so far (floor(n M / L) + K/2 < samples in); final[j] = 1 (final may be NULL: none) also emits
 * the rest, the input taken as zero past its end - the stream's outputs then number ft_resampled_len(rate, samples in) -
 * and closes the stream (a later chunk is FT_ERR_STATE).  lens[j] = 0 is allowed with final[j] = 1 (the tail alone).
 * audio: the streams' outputs back to back, out_lens[j] samples each; stream j emits at most
 * ft_resampled_len(rate, samples in after the chunk) minus what it emitted before.  A 44100 stream emits its chunk's
 * samples as ft_codec_stream_decode_many does (final changes nothing there).  Each stream's samples do not depend on
 * the chunking or on the other streams of the call.  Refusals (FT_ERR_ARG, FT_ERR_STATE, FT_ERR_TOO_LONG) as
 * ft_codec_stream_decode_many, before any device work, every stream unchanged. */
ft_status ft_codec_stream_decode_many_at(ft_ctx* ctx, int32_t n, ft_codec_stream* const* streams, const int32_t* codes,
                                         const int32_t* lens, const int32_t* final, float* audio, int64_t* out_lens);
/* Speaking rate.  The model draws its own durations, so these calls change the pace of the codec's waveform instead: a
 * pitch-preserving time-scale stage (WSOLA, waveform-similarity overlap-add) on the device, at the codec's 44100 Hz,
 * between the codec and the resampler.  speed_pct is an integer percentage in [50, 200] (anything else: FT_ERR_ARG before
 * any device work); 100 means the stage is absent, and the call is then ft_codec_decode_at / ft_codec_stream_begin_at.
 * The algorithm, with N = 1024 (window), HS = 512 (synthesis hop), D = 384 (alignment tolerance, +-8.7 ms) and
 * w[i] = 0.5 (1 - cos(2 pi i / N)), so that w[i] + w[i + HS] = 1:
 *   the input is x[0 .. n_in), zero outside; n_out = ceil(100 n_in / pct); frames k = 0 .. K-1, K = ceil(n_out / HS) + 1;
 *   a_k = floor(k HS pct / 100); frame k reads x[s_k + i], i in [0, N), s_k = a_k - HS + d_k, and adds w[i] x[s_k + i]
 *   to output (k - 1) HS + i (positions below 0 or from n_out on are dropped);
 *   d_0 = 0; for k >= 1, d_k is the d in [-D, D] that maximises c(d) = sum_{i<N} x[a_k - HS + d + i] x[s_{k-1} + HS + i],
 *   the plain cross-correlation with the natural continuation of frame k - 1; the lowest d wins a tie.  The sums are
 *   float32 (fused multiply-adds), over i ascending.
 * Emission (what makes the chunking irrelevant): a stream runs frame k once the input seen so far reaches
 * max(a_k, a_{k-1} + HS) + HS + D - the end of the frame's search region and of its template, the latter lying further on
 * below speed 1; after frame k the outputs below k HS are final and are emitted.  final runs the remaining frames with
 * zeros past the end; the stream's outputs then number n_out exactly.  A stream carries on the device the input samples a
 * later frame can still read (at most N + 2 D + 2 HS), s_{k-1} and the HS half-overlapped outputs, two copies each (a call
 * reads one and writes the other); k and the sample counters live on the host (csrc/fx_chain.h holds the host arithmetic
 * of all three output stages).  With a sample rate as well, the
 * resampler runs over the time-scaled samples (its input count is theirs).  The first time-scaled call allocates the
 * stage's buffers for speed 0.5: 2 max_frames frame_len float32 (plus 64 streams' hold-back), and a resampler output
 * buffer for that many input samples. */
/* Host only: ceil(100 n_in / speed_pct); -1 for a refused speed_pct. */
int64_t ft_timescaled_len(int32_t speed_pct, int64_t n_in);
/* ft_codec_decode_at at speed_pct: out_lens[b] = ft_resampled_len(sample_rate, ft_timescaled_len(speed_pct, lens[b] *
 * frame_len)); audio: B x max(out_lens) float32 (host).  ft_codec_decode_at is this call with speed_pct = 100. */
ft_status ft_codec_decode_fx(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                             int32_t sample_rate, int32_t speed_pct, float* audio, int64_t* out_lens);
/* ft_codec_stream_begin_at at speed_pct.  ft_codec_stream_decode_many_at serves such streams, mixed with any others in one
 * call (one workgroup of the stage per time-scaled stream); final and tail-only chunks behave as for the resampler, also at
 * 44100.  ft_codec_stream_decode and ft_codec_stream_decode_many refuse them (FT_ERR_STATE). */
ft_status ft_codec_stream_begin_fx(ft_ctx* ctx, int32_t sample_rate, int32_t speed_pct, ft_codec_stream** out);
/* Pitch.  A plain pitch shift of the codec's waveform by pitch_cents, an integer in [-1200, 1200] (anything else:
 * FT_ERR_ARG before any device work); 0 means the stage is absent, and the call is then ft_codec_decode_fx /
 * ft_codec_stream_begin_fx.  Formants move with the pitch (no formant preservation).  The shift is the two stages above put
 * together: stretch the waveform by the pitch ratio at unchanged pitch, then read it back faster by the same ratio.
 *   Step: S = llround(2^20 2^(cents / 1200)), computed in double; r = S / 2^20 is the realised pitch ratio (within half a
 *   step, 2^-21, of the nominal one: at most 2^-20 = 9.6e-7 relative, at r = 0.5; below 5e-7 from r = 1 on).
 *   Chain: codec -> time-scale stage -> pitch stage -> rate resampler, all on the codec's stream.
 *   Time-scale stage under pitch: the WSOLA algorithm above at the rational rate num / den, num = speed_pct 2^20,
 *   den = 100 S (speed_pct = 100 when no speed is given): a_k = floor(k HS num / den), and the stage's output count is
 *   ceil(n_in den / num).  A speed alone is num = pct, den = 100.  (64-bit arithmetic: k 512 200 2^20 < 2^52 within
 *   max_frames.)
 *   Accepted combinations: 50 S <= speed_pct 2^20 <= 200 S, which keeps the effective time-scale rate in [0.5, 2]; anything
 *   else is FT_ERR_ARG before any device work.  When speed_pct 2^20 == 100 S - (200, +1200) and (50, -1200) - the time-scale
 *   stage is absent and the pitch stage reads the codec's samples directly: a plain "play faster, higher".
 *   Pitch stage: output n is its input at time n S / 2^20.  With u = n S, i0 = u >> 20, p = (u >> 11) & 511,
 *   f = (u & 2047) / 2048:
 *     y[n] = sum_{t < K} ((1 - f) w[p][t] + f w[p + 1][t]) x[i0 - K/2 + 1 + t],
 *   in float32 over t ascending, in the same order whatever the chunking and however many segments share the launch.  The
 *   table w[513][K] is float32: a Kaiser-windowed sinc designed on the host in float64 with the resampler's constants
 *   (A = 75 dB, beta = 0.1102 (A - 8.7), transition 0.07), cut-off fc = 0.465 min(1, 1 / r) cycles per input sample,
 *   K = the even ceiling of (A - 7.95) / (2.285 2 pi 0.07) max(1, r) (68 taps for r <= 1, 134 at r = 2); tap w[p][t] is the
 *   prototype h(tau) = 2 fc sinc(2 fc tau) I0(beta sqrt(1 - (tau / (K/2))^2)) / I0(beta) (sinc(v) = sin(pi v) / (pi v)) at
 *   tau = p / 512 + (K/2 - 1 - t) input samples; row 512 is row 0 shifted by one tap.  One table per cents value, uploaded
 *   on first use and kept.  Through the interpolated coefficients the pass band to 0.43 min(1, 1 / r) is within 0.01 dB
 *   and the stop band from 0.5 / r is at least 70 dB down (measured in float64 on the float32 table: <= 0.0015 dB, >= 80 dB).
 *   Output length: the pitch stage emits exactly ft_timescaled_len(speed_pct, n_codec) samples, its input taken as zero
 *   past its end (the last output's centre tap lies at most two samples past it).  Pitch never changes an utterance's
 *   length: ft_resampled_len(rate, ft_timescaled_len(pct, n)) stays the length formula of every path.
 *   Streams: a pitched stream carries, besides the above, the stage's last K input samples (two copies: a call reads one
 *   and writes the other), its input and output counters on the host, and the time-scale state at the rational rate.  A
 *   chunk emits the outputs whose taps all lie within the stage's input seen so far ((n S >> 20) + K/2 < samples in);
 *   final emits the rest up to the exact length above and closes the stream; tail-only chunks work as for the resampler.
 *   A stream's samples depend neither on the chunking nor on the other streams of the call.
 *   The first pitched call allocates the time-scale stage's buffers (sized for rate 0.5, as its own first call does) and a
 *   pitch output buffer of the same size. */
/* Host only (no context, no device): S, K (K = 0 at 0 cents) and, if `table` is non-null, the 513 x K weights.  Any pointer
 * may be NULL.  FT_ERR_ARG outside [-1200, 1200], the outputs left untouched. */
ft_status ft_pitch_filter(int32_t cents, int64_t* step, int32_t* K, float* table);
/* Host only: FT_OK when (speed_pct, cents) is an accepted combination (speed_pct = 100: no speed), else FT_ERR_ARG. */
ft_status ft_pitch_ok(int32_t speed_pct, int32_t cents);
/* ft_codec_decode_fx at pitch_cents (same lengths, same layout); ft_codec_decode_fx is this call at 0 cents. */
ft_status ft_codec_decode_fxp(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                              int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents, float* audio, int64_t* out_lens);
/* ft_codec_stream_begin_fx at pitch_cents.  ft_codec_stream_decode_many_at serves such streams, mixed with any others in
 * one call; ft_codec_stream_decode and ft_codec_stream_decode_many refuse them (FT_ERR_STATE). */
ft_status ft_codec_stream_begin_fxp(ft_ctx* ctx, int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents,
                                    ft_codec_stream** out);
/* Join.  The utterances of one call - the sentences of a long text - trimmed to their loud part, faded at the cuts and laid
 * out behind pauses as ONE waveform, on the device, at the end of the chain: codec -> time-scale stage -> pitch stage ->
 * rate resampler -> join, all on the codec's stream.  The reference speaks a text as one utterance and has no such stage
 * (generate_long, inference.py:741-846, does not split the text).  The stage, which fixes every bit of its result:
 *   Inputs: item b has samples x_b[0 .. n_b), float32, at the output rate; ft_join_params {threshold >= 0, hop H >= 1,
 *   keep >= 0, fade F >= 0} (sample counts at the output rate); gaps[b] >= 0 samples; started in {0, 1}: audio of the same
 *   document went out before this call.
 *   Edges: window j of item b covers [j H, min((j + 1) H, n_b)), j = 0 .. ceil(n_b / H) - 1.  A window is loud when a sample
 *   of it has |x| >= threshold, compared in float32 (a NaN is never loud).  first / last = the lowest / highest loud window.
 *   No loud window: a_b = e_b = 0, the item contributes nothing.  Else a_b = max(0, first H - keep),
 *   e_b = min(n_b, (last + 1) H + keep); m_b = e_b - a_b.
 *   Fades: f_b = min(F, m_b / 2) (integer division).  Piece sample i is x_b[a_b + i]; for i < f_b it is multiplied by
 *   ramp(i), for i >= m_b - f_b by ramp(m_b - 1 - i), ramp(j) = (float)((double)(2 j + 1) / (double)(2 f_b)): one float32
 *   multiply per faded sample and nothing else touches a sample (the two ramps never overlap).
 *   Layout: s_b = started || any m_c > 0 for c < b; G_b = gaps[b] if m_b > 0 and s_b, else 0 (gap b comes before piece b; it is
 *   dropped for an empty piece and before the first audio of the document); off_b = sum_{c < b} (G_c + m_c).  The output
 *   holds G_b zeros (+0.0) at off_b, then the piece; total = sum (G_b + m_b).
 *   Outputs: audio[0 .. total), total and cuts[b] = (a_b, e_b).
 * With threshold = 0, keep = 0, fade = 0 the join is plain concatenation with gaps; a piece depends on its own item only, so
 * the items of a document may be split over several calls, `started` carried (1 once a call returned total > 0).
 * Three launches whatever B (edges, layout, assemble; the item is a grid dimension), then two copies to the host: total
 * with the cuts (1 KB), and `total` samples - one audio copy per call, not one per item. */
typedef struct ft_join_params {
    float threshold;           /* linear amplitude */
    int32_t hop, keep, fade;   /* samples at the output rate */
} ft_join_params;
/* ft_codec_decode_fxp with the items joined on the device: item b's samples before the join are, bit for bit, row b of
 * ft_codec_decode_fxp for the same arguments (out_lens[b] of them).  Limits: 1 <= B <= 64, lens[b] >= 0 (lens NULL: T each),
 * sum(lens) <= max_frames.  capacity = the room in `audio` (samples); it must be at least sum(out_lens) + sum(gaps).
 * audio receives `total` samples (nothing past them is written), *total their number, cuts B x 2 the (a_b, e_b).  Every
 * argument is checked before any device work: FT_ERR_ARG (a bad rate, speed, pitch or combination; B outside [1, 64]; a null
 * pointer; a length outside [0, T]; bad join parameters; a negative gap; started not 0 or 1; capacity too small;
 * more than 2^28 samples of items and gaps), FT_ERR_TOO_LONG (T or sum(lens) beyond max_frames).  The first call allocates the
 * stage's table (64 items, < 8 KB) and, besides what ft_codec_decode_fxp allocates for the same arguments, an input buffer
 * of sum(out_lens) (every item rounded up to 4 samples) and an output buffer of sum(out_lens) + sum(gaps) float32; a later
 * call that needs more replaces them by larger ones. */
ft_status ft_codec_decode_join(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                               int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents, const ft_join_params* jp,
                               const int64_t* gaps, int32_t started, float* audio, int64_t capacity, int64_t* total,
                               int64_t* cuts);
/* Host only (no context, no device): consecutive items of lens[i] code frames grouped into ft_codec_decode_join calls of at
 * most 64 items and max_frames frames; ends[g] (room for n) = one past the last item of group g.  Returns the number of
 * groups, -1 for a negative length, an item beyond max_frames or a null pointer. */
int32_t ft_join_groups(const int32_t* lens, int32_t n, int32_t max_frames, int32_t* ends);
/* Level.  The model sets its own level per utterance; these calls bring every item to a caller-chosen integrated loudness
 * (ITU-R BS.1770-4 / EBU R128) on the device, as the last stage of the chain and in front of the join:
 * codec -> time-scale stage -> pitch stage -> rate resampler -> level -> (join), all on the codec's stream.  The reference
 * has no such stage.  The stage runs at the output rate Fo; per item it measures the integrated loudness and the sample
 * peak, derives ONE gain and multiplies every sample of the item by it.  Stated, which fixes its result:
 *   Inputs: item b has samples x[0 .. n), float32, at rate Fo.  The target T is in LUFS, given as an integer number of
 *   hundredths (`loudness`): accepted values are [-5000, -500]; 0 means the stage is absent (the call is then the one without
 *   it, bit for bit); anything else is FT_ERR_ARG before any device work.  The ceiling c = 10^(-1/20), -1 dBFS on the sample
 *   peak, is fixed.
 *   K-weighting at any rate: two biquads in series, designed in float64 on the host from the analogue prototypes (at 48 kHz
 *   they are the table of BS.1770 to 1e-12).
 *     Shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / Fo), Vh = 10^(G/20),
 *     Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2; b = [(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0],
 *     a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0].
 *     High-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, K = tan(pi f0 / Fo), d = 1 + K/Q + K^2; b = [1, -2, 1],
 *     a = [1, 2 (K^2 - 1)/d, (1 - K/Q + K^2)/d].
 *   z = hp(shelf(x)), both filters from zero state at sample 0.  The recursion and every sum below run in float64.
 *   Blocks: the hop is H = floor(Fo / 10).  Hop sums e_h = sum z^2 over [h H, (h + 1) H), h < floor(n / H).  Block j is
 *   E_j = (e_j + e_{j+1} + e_{j+2} + e_{j+3}) / (4 H), j = 0 .. floor(n / H) - 4: whole 400 ms blocks only, overlapped by
 *   75 %.  An item shorter than 4 H with n >= 1 has the single block E_0 = sum z^2 / n.  l_j = -0.691 + 10 log10 E_j.
 *   Gates: the absolute gate keeps blocks with l_j > -70.  If none is kept, or n = 0, or a sum is not finite, L = -inf and
 *   the gain is exactly 1.  The relative gate is Gamma = -0.691 + 10 log10(mean E_j over the absolute-gated) - 10, and
 *   L = -0.691 + 10 log10(mean E_j over the blocks with l_j > -70 and l_j > Gamma).
 *   Gain: p = max |x|; g = min(10^((T/100 - L)/20), c / p) in float64 (no ceiling term when p = 0), rounded once to float32.
 *   Output sample i is the float32 product g x[i]: one multiply and nothing else.
 *   Reported per item (ft_level_info): L, p, g, the number of blocks, the number that passed both gates, and whether the
 *   ceiling bound the gain.
 *   Determinism: no floating-point atomics; every sum runs in a fixed order, so a call repeated gives the same bits.
 * On the device the recursion runs one lane per hop, each lane starting both filters from zero state 2 H samples (0.2 s)
 * before its hop, or at sample 0: the high-pass's double pole has decayed by e^-48 over that stretch at every rate, which
 * leaves z within 1e-13 of the recursion from sample 0 (measured in float64 on noise with a DC offset); the hop sums do not
 * depend on how the lanes are spread over the grid.  Three launches whatever the number of items (filter, gates and gain,
 * multiply; the item is a grid dimension).  The first levelled call allocates the stage's table (64 items, < 4 KB) and one
 * float64 and one float32 per hop of the call's items; a later call that needs more replaces them by larger ones.
 * No stream entry point takes a level: the integrated loudness of an utterance is not known before its end.  A stream is
 * levelled by the ride stage instead (ft_codec_stream_begin_live, below). */
typedef struct ft_level_info {
    double lufs;               /* L: integrated loudness; -inf when nothing was measured (the gain is then 1) */
    float peak, gain;          /* p = max |x| of the item before the stage; g */
    int32_t blocks, gated;     /* 400 ms blocks of the item; those that passed both gates */
    int32_t capped;            /* 1: the ceiling bound the gain (g = c / p) */
} ft_level_info;
/* Host only (no context, no device): validates the rate as ft_resample_filter does (FT_ERR_ARG otherwise, the outputs left
 * untouched); coeffs[10] = the shelf's b0 b1 b2 a1 a2, then the high-pass's; *hop = H.  Either pointer may be NULL. */
ft_status ft_level_filter(int32_t sample_rate, double* coeffs, int32_t* hop);
/* The stage alone on a host waveform x of n >= 0 samples at sample_rate - this is also how a caller measures a reference
 * clip.  target = 0 measures only (gain 1); y (may be NULL: nothing is multiplied or copied) receives the n levelled samples.
 * n may be as long as the longest item a decode gives (max_frames frames at speed 0.5 and 48000 Hz), FT_ERR_TOO_LONG beyond.
 * FT_ERR_ARG before any device work: a refused rate, a target that is neither 0 nor in [-5000, -500], a null x or info. */
ft_status ft_codec_loudness(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, int32_t target,
                            ft_level_info* info, float* y);
/* ft_codec_decode_fxp with the level stage behind the resampler: row b is, bit for bit, ft_codec_loudness at `loudness` over
 * row b of ft_codec_decode_fxp (its out_lens[b] samples; zeros past them as there).  infos (B entries; may be NULL) receives
 * every item's result.  ft_codec_decode_fxp is this call at loudness = 0. */
ft_status ft_codec_decode_level(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents, int32_t loudness, float* audio,
                                int64_t* out_lens, ft_level_info* infos);
/* ft_codec_decode_join with the level stage in front of the join: every item is levelled on its own, all of them in one go,
 * before the edges are found - the join's threshold therefore acts on the levelled samples, which gives its absolute figure
 * a meaning.  The result is ft_test_join over the rows of ft_codec_decode_level.  infos (B entries; may be NULL) as there.
 * ft_codec_decode_join is this call at loudness = 0. */
ft_status ft_codec_decode_join_level(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                     int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents, int32_t loudness,
                                     const ft_join_params* jp, const int64_t* gaps, int32_t started, float* audio,
                                     int64_t capacity, int64_t* total, int64_t* cuts, ft_level_info* infos);
/* ft_codec_decode_join_level with a chain per item - the lines of a script, each at its own pace, pitch and level, in one
 * waveform: item b goes through fx[b] (B entries; the values as ft_codec_decode_level takes them).  One output rate per
 * call, because the result is one waveform.  What fixes the result: before the join, item b's samples are, bit for bit, row b
 * of ft_codec_decode_level(sample_rate, fx[b].speed_pct, fx[b].pitch_cents, fx[b].loudness) for the same codes, and the
 * output is ft_test_join over those rows with jp, gaps and started.  With all fx[b] equal the call is
 * ft_codec_decode_join_level, bit for bit.  An item with loudness = 0 is not levelled and its infos[b] (infos may be NULL)
 * is the empty result {-inf, 0, 1, 0, 0, 0}; the levelled items are levelled in one go, each toward its own target: three
 * launches whatever B.  No kernel is new here: the stages are those above, driven per item, and the level stage reads its
 * target from the item.  Before the first decode the call builds the pitch table of every distinct cents value, allocates
 * the buffers of its longest chain and the hop sums of its levelled items.  Every argument is checked before any device
 * work, in this order, and a refused call changes nothing: the rate; then for each item in order its speed, cents, pair and
 * level as ft_codec_decode_level judges them (FT_ERR_ARG, the message names the item); then the checks of
 * ft_codec_decode_join, out_lens[b] being that of item b's own chain. */
typedef struct ft_item_fx {
    int32_t speed_pct, pitch_cents, loudness;
} ft_item_fx;
ft_status ft_codec_decode_join_items(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                     int32_t sample_rate, const ft_item_fx* fx, const ft_join_params* jp,
                                     const int64_t* gaps, int32_t started, float* audio, int64_t capacity, int64_t* total,
                                     int64_t* cuts, ft_level_info* infos);
/* Ride.  A stream cannot wait for its integrated loudness, so it gets a second, streaming level stage: a look-ahead gain
 * rider with carried state, last in the stream's chain: codec -> time-scale stage -> pitch stage -> rate resampler -> ride.
 * It is a different operation from the level above - a gain that varies in time, steered by the loudness of the programme
 * so far - and its output does not depend on how the stream was cut into chunks, bit for bit, like the other three stream
 * stages.  The measure is cumulative: after a change of level the output settles toward the loudness of the programme so
 * far and does not pump (a 6.4 s signal with a +12 dB step came out at -21.3 LUFS overall for a -23 target); that is
 * intended.  Stated, which fixes its result:
 *   Inputs: a stream's samples x[0 .. n) at the output rate Fo, float32, arriving in chunks; n is known only at `final`.
 *   The target T (`live`) is in hundredths of a LUFS in [-5000, -500]; 0 means the stage is absent (the call is then the one
 *   without it, bit for bit); anything else is FT_ERR_ARG before any device work.
 *   Constants: the level stage's hop H = floor(Fo / 10) and ceiling c = 10^(-1/20); look-ahead A = 10 hops; slew R = 0.5 dB
 *   per hop.
 *   Hop sums and peaks: z is the K-weighted x exactly as the level stage computes it (the same design, float64, one lane
 *   per hop from zero state 2 hops earlier or at sample 0).  e_h = sum z^2 over [h H, (h + 1) H) for the W = floor(n / H)
 *   whole hops; p_h = max |x| over hop h for h < Nh = ceil(n / H), the last one over what is left; p_-1 = p_Nh = 0.
 *   Running measure: L(m) is the level stage's integrated loudness of the first m whole hops (its blocks and gates over
 *   e_0 .. e_m-1 as an item of m H samples: 400 ms blocks, both gates, a single mean block below four hops, -inf when
 *   nothing passes).
 *   Nodes: node k sits at sample k H, k = 0 .. Nh.  m_k = min(k + A, W).  u_k = T / 100 - L(m_k) when L(m_k) is finite,
 *   else u_k = v_k-1 (v_-1 = 0).  v_0 = u_0; for k >= 1, v_k = min(max(u_k, v_k-1 - R), v_k-1 + R).  Peak guard:
 *   q_k = max(p_k-1, p_k), cap_k = 20 log10(c / q_k), +inf when q_k = 0; the guard does not feed back into v.
 *   g_k = (float) 10^(min(v_k, cap_k) / 20): float64 throughout, rounded to float32 once.
 *   Output: for i = k H + j, 0 <= j < H: y[i] = x[i] * fmaf((float)j / (float)H, g_k+1 - g_k, g_k), float32 with an IEEE
 *   division, and nothing else touches a sample.  Both nodes of hop k are at most c / p_k, so |y| <= c up to rounding.
 *   Silence, or nothing above the gates, gives g = 1 exactly and y = x bit for bit.
 *   Emission: after n_in samples with W' = floor(n_in / H) whole hops, node k is final once k + A <= W', and the outputs
 *   below max(0, W' - A) H are final and are emitted.  `final` computes the remaining nodes with m_k = min(k + A, W) and
 *   emits all n samples.  The stage changes no length; a stream holds back less than (A + 1) H samples.
 *   Determinism: no floating-point atomics; every reduction runs in an order that depends only on m_k, never on the call.
 * On the device a stream carries the held-back samples (two copies: a call reads one and writes the other), its hop sums,
 * peaks, nodes and v; the counters live on the host.  Three launches per call whatever the number of streams (the hops the
 * call completes; the new nodes, one workgroup per stream; the multiply and the roll of the carry).  A live stream's first
 * audio comes A hops (one second) of output later than a plain stream's.  A stream that rolls over at max_frames, or is cut
 * by the caller's max_tokens, starts a fresh ride state with its fresh codec stream: the level is not carried over that one
 * boundary. */
/* Host only (no context, no device): validates the rate as ft_resample_filter does (FT_ERR_ARG otherwise, or for n_in < 0).
 * After n_in samples of a stream (final: its end), *nodes = the nodes that are final and *n_out = the samples emitted so
 * far.  Either pointer may be NULL. */
ft_status ft_ride_plan(int32_t sample_rate, int64_t n_in, int32_t final, int64_t* nodes, int64_t* n_out);
/* The stage alone on a host waveform x of n >= 0 samples at sample_rate, as one stream whose only call is its last.  y
 * receives the n samples; nodes (may be NULL) receives the ceil(n / H) + 1 nodes g_k.  target = 0: y = x, every node 1.
 * Limits and refusals as ft_codec_loudness: n up to the longest item a decode gives, FT_ERR_TOO_LONG beyond; FT_ERR_ARG
 * before any device work for a refused rate, a target that is neither 0 nor in [-5000, -500], a null x or y. */
ft_status ft_codec_ride(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, int32_t target, float* y, float* nodes);
/* ft_codec_stream_begin_fxp with the ride stage behind the resampler at target `live`; with live = 0 it is that call.
 * ft_codec_stream_decode_many_at serves such streams, mixed with any others in one call: the concatenation of a stream's
 * chunks is, bit for bit, ft_codec_ride over the concatenation of the same stream opened without the target.
 * ft_codec_stream_decode and ft_codec_stream_decode_many refuse them (FT_ERR_STATE); ft_codec_stream_end frees the state:
 * two carries of (A + 1) H floats and 24 bytes per 100 ms of the longest stream (max_frames frames at speed 0.5). */
ft_status ft_codec_stream_begin_live(ft_ctx* ctx, int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents, int32_t live,
                                     ft_codec_stream** out);
/* Codec encode = vocoder.encode(audio, lengths) of encode_reference (synthesizer.py:325-357, vocoder.py:885-904):
 * mono f32 audio at the codec sample rate (host), right-padded to whole frames -> codes (num_codebooks+1) x T'
 * int32 row-major (host, row stride = T' = ceil(n_samples / ft_codec_enc_frame_len)); *out_frames = T'. */
ft_status ft_codec_encode(ft_ctx* ctx, const float* audio, int64_t n_samples, int32_t* codes, int32_t* out_frames);
int32_t ft_codec_enc_frame_len(const ft_ctx* ctx);
/* Reference intake.  A cloned voice is as good as what the encoder is given; these calls take the frames of a WAV as they lie
 * in the file and prepare them on the device, on the codec's stream: raw bytes -> intake (decode, mix down, resample to
 * 44100 Hz; one launch for all clips of a call) -> level -> trim and fades (the join stage) -> encoder.  The reference reads
 * 16-bit mono only, resamples with a whole-clip FFT on the host and keeps silence and level as they come
 * (synthesizer.py:613-631); ft_codec_encode is that path and is unchanged.  Stated, which fixes every bit of the result:
 *   Inputs: item b = {data, n_frames >= 1, rate, channels in [1, 8], fmt, channel}: n_frames frames of `channels` interleaved
 *   little-endian samples (host memory, no alignment asked); fmt 0 u8, 1 s16, 2 s24 (three bytes), 3 s32, 4 f32; channel = -1
 *   takes the mean of all channels, channel = k in [0, channels) takes channel k alone.
 *   Samples: channel sample v becomes the real number d = (v - 128) / 128 (u8), v / 32768 (s16), v / 8388608 (s24),
 *   v / 2147483648 (s32), v itself (f32; a v that is not finite counts as 0).  The mono sample of frame i is
 *   m[i] = (float)(sum_c d_c / C): the sum in float64 over c ascending (exact), one float64 division, rounded once to float32;
 *   with channel = k it is (float) d_k.  m is zero outside [0, n_frames).  A 16-bit mono file gives v / 32768 exactly.
 *   Rate: Fi = rate, Fo = 44100; g = gcd(Fi, 44100), L = 44100 / g, M = Fi / g, Fmin = min(Fi, 44100).  The filter is the
 *   resampler's (ft_resample_filter) designed for this pair: A = 75 dB, beta = 0.1102 (A - 8.7), K = the even ceiling of
 *   (A - 7.95) / (2.285 2 pi 0.07) Fi / Fmin, cut-off 0.465 Fmin / (L Fi) cycles per sample at the up-sampled rate L Fi, gain L,
 *   tap t of phase p the prototype at p + (K/2 - 1 - t) L; pass band to 0.43 Fmin (<= 0.01 dB), stop band from 0.5 Fmin
 *   (>= 70 dB).  Accepted rates: integers in [8000, 192000] with L <= 640 and (255 M + L - 1) / L + K + 1 <= 2048 (8000, 11025,
 *   12000, 16000, 22050, 24000, 32000, 48000, 64000, 88200, 96000, 176400, 192000 among them: K from 68 to 292).  At 44100,
 *   K = 0 and y[n] = m[n].  Else n44 = ceil(n_frames L / M) outputs, y[n] = sum_{t < K} w[p][t] m[i0 - K/2 + 1 + t] with
 *   u = n M, i0 = u / L, p = u % L, in float32 over t ascending.  An output does not depend on the other clips of the call.
 *   Counters (exact integers, over the channels that are used): clipped = samples at an extreme code of their format (0 or
 *   255; -32768 or 32767; ...), for f32 finite samples with |v| >= 1; nonfinite = f32 samples that are not finite (they are
 *   not counted as clipped).
 *   Level: the level stage (ft_codec_loudness) over every clip's n44 samples at 44100 Hz.  It always measures - infos[b].level
 *   holds L and the peak of the clip before the gain - and multiplies by the gain only with a target (`loudness` in
 *   [-5000, -500]; 0: the clip keeps its level, the reported gain is 1).
 *   Trim: the join stage (ft_codec_decode_join) over the levelled clips with jp, every gap 0 and started = 0: piece b is
 *   x_b[a_b .. e_b) with its fades, m_b = e_b - a_b samples; the pieces lie back to back.  With threshold = 0, keep = 0,
 *   fade = 0 nothing is trimmed or faded and m_b = n44_b.
 *   Encoder: piece b is encoded as ft_codec_encode encodes the same samples from the host, bit for bit, wherever
 *   1 <= m_b <= max_enc_frames * ft_codec_enc_frame_len; frames_b = ceil(m_b / ft_codec_enc_frame_len).
 *   Reported per item (ft_intake_info): n44, (a, e), frames, the two counters, the level, and status: 0 ok; 1 no loud window
 *   (m_b = 0: nothing kept, nothing encoded); 2 the kept piece is longer than the encoder takes (not encoded: cutting it
 *   would leave its transcript behind).  frames = 0 unless status = 0.  Items with status 1 or 2 do not fail the call.
 * Limits: 1 <= B <= 64; n44 <= the level stage's longest item (ft_codec_loudness); raw bytes of a call (every item rounded
 * up to 16) <= 2^30; sum(n44) <= 2^28.  Every argument is checked before any device work, and a refused call changes
 * nothing: FT_ERR_ARG (a null pointer; B; n_frames < 1; fmt; channels; channel >= channels or < -1; a refused rate; a loudness
 * that is neither 0 nor in [-5000, -500]; bad join parameters; capacity too small), FT_ERR_TOO_LONG (n44 or the raw bytes
 * beyond the limits), FT_ERR_STATE (ft_codec_encode_items on a context without the encoder).
 * On the device: the raw bytes lie in one buffer, every clip on a 16-byte boundary (a 24-bit clip with an odd number of
 * frames would leave its successor unaligned otherwise); the clips at 44100 Hz lie in the join stage's input buffer, the
 * pieces in its output buffer; one [L][K] table per input rate, uploaded on first use and kept (168 KB at most).  The buffers
 * grow when a later call needs more.  Launches per call: 1 (intake) + 2 or 3 (level) + 3 (join), whatever B; then one
 * read-back of the cuts, the encoder clip by clip on the stream, all codes gathered on the device and copied once. */
typedef struct ft_intake_item {
    const void* data;
    int64_t n_frames;
    int32_t rate, channels, fmt, channel;
} ft_intake_item;
typedef struct ft_intake_info {
    int64_t n44, a, e;
    int32_t frames, status;
    int64_t clipped, nonfinite;
    ft_level_info level;
} ft_intake_info;
/* Host only (no context, no device): the intake filter of rate_in; L, M, K (K = 0 at 44100) and, if `table` is non-null, the
 * L x K weights.  Any output pointer may be NULL.  FT_ERR_ARG for a refused rate, the outputs left untouched. */
ft_status ft_intake_filter(int32_t rate_in, int32_t* L, int32_t* M, int32_t* K, float* table);
/* ceil(n L / M) - the samples n frames at rate_in give at 44100 Hz; -1 for a refused rate or n < 0. */
int64_t ft_intake_len(int32_t rate_in, int64_t n);
/* The prepared pieces themselves - what the encoder would be given - back to back in `audio` (host), lens[b] = m_b samples
 * each; capacity (samples) must be at least sum(n44).  Needs no encoder: without one frames = 0 and status 2 does not
 * arise; with one, infos are those of ft_codec_encode_items for the same arguments. */
ft_status ft_codec_intake(ft_ctx* ctx, int32_t B, const ft_intake_item* items, const ft_join_params* jp, int32_t loudness,
                          float* audio, int64_t capacity, int64_t* lens, ft_intake_info* infos);
/* The codes of every item with status 0, back to back in `codes` (host): item b's block is (n_codebooks+1) x frames_b int32
 * row-major.  capacity_frames must be at least sum_b ceil(n44_b / ft_codec_enc_frame_len), the most the call can give. */
ft_status ft_codec_encode_items(ft_ctx* ctx, int32_t B, const ft_intake_item* items, const ft_join_params* jp,
                                int32_t loudness, int32_t* codes, int64_t capacity_frames, ft_intake_info* infos);
/* Mix.  A music bed under a finished programme: codec -> time-scale stage -> pitch stage -> rate resampler -> level -> join ->
 * mix.  The bed is a second WAV, prepared by the intake launches, brought to the output rate, looped or cut to the
 * programme's length, lowered by a look-ahead sidechain gain that follows where the programme is loud, added to the programme
 * and held under the -1 dBFS ceiling, all on the codec's stream.  The reference has no such stage.  Stated, which fixes every
 * bit of the result:
 *   Inputs: the programme x[0 .. n), float32 at the output rate Fo (any rate ft_resample_filter accepts), n >= 1; the bed, one
 *   ft_intake_item (its `channel` field is not read: mp->channel stands for it); ft_mix_params, sample counts at Fo:
 *   bed_loudness 0 or in [-5000, -500] hundredths of a LUFS (the intake's `loudness`), channel (the intake's), depth in
 *   [0, 6000] hundredths of a dB, threshold >= 0 (linear), attack Wa and release Wr in hops, each in [1, 500], lead and tail
 *   >= 0 (bed alone before and after the programme), fade_in and fade_out >= 0, offset >= 0 (the first bed sample used),
 *   loop 0 or 1.
 *   Bed: bed44 is, bit for bit, the piece ft_codec_intake gives for the item with jp = (0, 1, 0, 0) and loudness =
 *   bed_loudness (nothing trimmed); bed is, bit for bit, what resample_kernel gives for the whole of bed44 from zero state in one
 *   final call (ft_test_resample), at Fo = 44100 bed44 itself.  Its length is nb; nb = 0 is refused with FT_ERR_ARG.
 *   Timeline: N = lead + n + tail; s[i] = x[i - lead] inside [lead, lead + n), else +0.0.  With j = i + offset, b(i) =
 *   bed[j mod nb] with loop; without it bed[j] for j < nb and +0.0 past it.
 *   Activity: H = floor(Fo / 50) (20 ms), Nh = ceil(N / H); act_h = some sample of [h H, min((h + 1) H, N)) has
 *   |s| >= threshold, compared in float32 (the join's rule: a NaN is never loud).  That is P_h >= threshold with P_h the
 *   largest |s| of the hop that is not a NaN.
 *   Duck: nodes k = 0 .. Nh at sample k H; D_k, an integer in hundredths of a dB, is the largest of 0,
 *   depth (Wa - (h - k)) / Wa over active h in [k, k + Wa - 1] and depth (Wr - (k - 1 - h)) / Wr over active h in
 *   [k - Wr, k - 1]; only hops in [0, Nh) count; integer divisions in int64.  So both nodes of an active hop sit at full
 *   depth, the gain falls over Wa hops before speech and rises over Wr hops after it; it is a function of the activity alone.
 *   Gains: g_k = T[D_k], T[d] = (float) 10^(-d / 2000) for d = 0 .. 6000, float64 rounded once (ft_mix_gains); T[0] = 1.
 *   Sample i = k H + j: r = (float) j / (float) H (an IEEE division), gd = fmaf(r, g_k+1 - g_k, g_k); t = b(i); if
 *   i < f_in = min(fade_in, N / 2), t = t ramp_in(i); if i >= N - f_out, f_out = min(fade_out, N / 2), t = t ramp_out(N - 1 - i);
 *   ramp(j) = (float)((double)(2 j + 1) / (double)(2 f)) with f the fade's length (the join's ramp); u = t gd; m[i] = s[i] + u.
 *   Every product and the sum are rounded to float32 on their own, none contracted.
 *   Ceiling: pk = max |m| (a NaN is never the peak), c = 10^(-1/20); if pk > c every sample is multiplied once by
 *   sg = (float)(c / pk) (float64, rounded once), else nothing more touches a sample.
 *   It follows: a bed of zeros gives `lead` zeros, x, `tail` zeros (a -0.0 of x becomes +0.0); depth = 0 gives every node
 *   exactly 1; a call repeated gives the same bits (no floating-point atomics; the peak is a max).
 *   Reported (ft_mix_info): N, nb, Nh, the active hops, the largest D_k, pk, sg (1 when not capped), capped, the bed's
 *   ft_intake_info.  duck (may be NULL) receives D_0 .. D_Nh.
 * Limits: N <= 2^28; the bed as an intake item; capacity >= N.  Every argument is checked before any device work and a
 * refused call changes nothing.  The checks, in this order: a null pointer (FT_ERR_ARG); sample_rate; n < 1; bed_loudness;
 * depth; threshold (a NaN too); attack; release; lead; tail; fade_in; fade_out; offset; loop (FT_ERR_ARG each);
 * n, lead, tail or N beyond 2^28 (FT_ERR_TOO_LONG); capacity < N (FT_ERR_ARG); then the bed as ft_codec_intake judges an
 * item: no frames, fmt, channels, channel, rate (FT_ERR_ARG), its length (FT_ERR_TOO_LONG).  A bed that comes out of the
 * intake with no sample (nb = 0) is refused after the intake launches (FT_ERR_ARG).
 * On the device: the programme, the bed at Fo, the output, one activity byte per hop, D_k and g_k per node; the buffers grow
 * when a later call needs more.  Launches beyond the bed's preparation (intake, level, join, resampler): mix_hop_kernel (hop
 * activity), mix_node_kernel (D_k, the flags of a workgroup's window staged in LDS), mix_kernel (the sample rule and the
 * peak), and mix_scale_kernel only when the ceiling binds. */
typedef struct ft_mix_params {
    int32_t bed_loudness, channel, depth;
    float threshold;
    int32_t attack, release;
    int64_t lead, tail, fade_in, fade_out, offset;
    int32_t loop, reserved;
} ft_mix_params;
typedef struct ft_mix_info {
    int64_t N, nb, Nh, active;
    int32_t dmax, capped;
    float pk, sg;
    ft_intake_info bed;
} ft_mix_info;
ft_status ft_codec_mix(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_intake_item* bed,
                       const ft_mix_params* mp, float* y, int64_t capacity, int64_t* total, int32_t* duck, ft_mix_info* info);
/* Host only: the timeline of a call - N = lead + n + tail, the hop H and the Nh + 1 nodes.  Any output pointer may be NULL.
 * FT_ERR_ARG / FT_ERR_TOO_LONG as ft_codec_mix judges the four values. */
ft_status ft_mix_plan(int32_t sample_rate, int64_t n, int64_t lead, int64_t tail, int64_t* N, int32_t* hop, int64_t* nodes);
/* Host only: T[0 .. 6000]. */
ft_status ft_mix_gains(float* table);
/* Stereo mix.  The mix stage with two channels out: the mono programme panned region by region - the lines of a script, each
 * at its speaker's place - and the two sides of the bed kept apart: codec -> ... -> join -> stereo mix.  Mix, its bits and its
 * refusals stay as they are; what this paragraph does not state is Mix's.  Stated, which fixes every bit of the result:
 *   Inputs: the programme x[0 .. n) as for ft_codec_mix; R pan regions, 0 <= R <= 4096, ft_pan_region {a, e, pan} each with
 *   0 <= a < e <= n, e_r <= a_r+1 (sorted, disjoint; they may touch) and pan in [-100, 100], -100 hard left; one bed item, or
 *   NULL; ft_mix_params with Mix's fields, checks and check order.  q(i) is the pan of the region that holds i - lead, 0 where
 *   none does.
 *   Pan table: U[j] = (float) min(1, sqrt(2) sin(j pi / 400)) for j = 0 .. 200, float64 rounded once; U[0] = 0 and U[j] = 1 for
 *   j >= 100 by definition (ft_pan_gains).  The right gain of pan q is P_1(q) = U[100 + q], the left one P_0(q) = U[100 - q]:
 *   constant power (P_0^2 + P_1^2 = 2 sin^2 + 2 cos^2 below the clamp) normalised to the centre, so that no gain exceeds 1 - a
 *   levelled voice keeps its ceiling - and a centred voice is the mono programme itself.
 *   Programme: s_c[i] = x[i - lead] P_c(q(i)), one float32 product, inside [lead, lead + n), +0.0 outside it.
 *   Bed sides: with mp->channel = -1 side 0 is channel 0 and side 1 is channel 1 of a file with two or more channels, channel 0
 *   of a mono file; with mp->channel = k both sides are channel k.  Where both sides name one channel the bed is Mix's mono bed
 *   for the same item and mp, bit for bit, level included, prepared once.  Else side c at 44100 Hz is, bit for bit, the piece
 *   ft_codec_intake gives for the item with channel = c, jp = (0, 1, 0, 0) and loudness 0.
 *   Pair level (only with bed_loudness != 0 and two different sides): e_h = e_h(side 0) + e_h(side 1), one float64 addition
 *   per hop of the level stage's own hop sums (the BS.1770 channel weights of left and right are 1), p = the larger of the
 *   two peaks; then the blocks, both gates, L and g exactly as the level stage states them for one item of n44 samples with
 *   those sums, and every sample of both sides is multiplied once by that one g in float32.  info->bed.level is the pair's.
 *   Each side then goes through resample_kernel on its own, from zero state, as in Mix; nb is common to both.
 *   Timeline, activity, D_k, g_k: Mix's, from the mono x - identical to ft_codec_mix for the same x and mp.
 *   Sample: m_c[i] is Mix's sample rule over s_c and b_c (the bed rule over side c): the fades, gd, every product and the sum
 *   rounded on its own.  Without a bed t = +0.0 and the rule runs as stated (nb = 0, info->bed zeroed; mp is still checked).
 *   Ceiling: pk = max |m_c| over both channels (a NaN is never the peak); one sg for both.
 *   Output: y[2 i + c], interleaved; capacity and *total count frames.
 *   It follows: with every q = 0 and equal sides y[2 i] = y[2 i + 1] = ft_codec_mix's y[i], bit for bit; with bed_loudness = 0
 *   channel c is, up to the ceiling, the mono call with channel = c over the programme s_c; a call repeated gives the same
 *   bits (no floating-point atomics).
 *   Reported: ft_mix_info as Mix reports it (N, nb, Nh in frames; pk, sg over both channels); with two different sides
 *   info->bed is side 0's ft_intake_info with the counters of both sides added and the pair's level (measured without a
 *   target too).
 * Limits and refusals: Mix's, in Mix's order, with the regions judged behind the rate and n: a null table with R > 0, R
 * outside [0, 4096], a region out of order or outside [0, n), a pan outside [-100, 100] (FT_ERR_ARG each).  Every argument is
 * checked before any device work and a refused call changes nothing.
 * On the device: Mix's buffers, the bed buffer holding both sides (each on a 16-byte boundary) and the output 2 N floats; the
 * pan table and the call's regions.  Launches beyond the bed's preparation: mix_hop_kernel and mix_node_kernel as they are,
 * mix_stereo_kernel (the sample rule for both channels and the peak; the regions that meet a workgroup's span found once per
 * workgroup and kept in LDS), mix_scale_kernel over the 2 N floats when the ceiling binds; for the pair level
 * level_pair_kernel, level_gain_kernel and level_pair_scale_kernel behind the intake's own launches. */
typedef struct ft_pan_region {
    int64_t a, e;
    int32_t pan, reserved;
} ft_pan_region;
ft_status ft_codec_mix_stereo(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_pan_region* regions, int32_t R,
                              const ft_intake_item* bed, const ft_mix_params* mp, float* y, int64_t capacity, int64_t* total,
                              int32_t* duck, ft_mix_info* info);
/* Host only: U[0 .. 200]. */
ft_status ft_pan_gains(float* table);
/* Room.  A convolution reverb behind the join: codec -> ... -> join -> room -> mix | stereo mix.  The programme, weighted
 * region by region by a send, is convolved with a room's impulse response (IR) in direct form and added to the dry programme.
 * The convolution runs on the f32-input MFMA, whose result is a k-ordered float32 fmaf chain, so the stage is stated to the
 * bit like Mix; an FFT convolution could not be.  Mix, Stereo mix and their live forms stay as they are.  Stated, which fixes
 * every bit of the result for finite inputs:
 *   Inputs: the programme x[0 .. n), float32 at Fo (any rate ft_resample_filter accepts), n >= 1; one IR item (its `channel`
 *   field is not read: rp->channel stands for it, -1 the mean of all channels, as in Mix); R send regions, 0 <= R <= 4096,
 *   ft_send_region {a, e, send} each with 0 <= a < e <= n, sorted and disjoint (they may touch); a send is an attenuation in
 *   hundredths of a dB in [0, 6000], or -1 for muted; s(i) is the send of the region that holds i, rp->send where none does.
 *   ft_room_params, sample counts at Fo: wet in [0, 6000], dry in [0, 6000] or -1 for no dry signal, predelay in [0, Fo],
 *   offset >= 0, length >= 0 (0: all of it), fade >= 0, tail >= -1, normalize and ceiling 0 or 1.
 *   Impulse response: ir44 is, bit for bit, the piece ft_codec_intake gives for the item with channel = rp->channel,
 *   jp = (0, 1, 0, 0) and loudness 0; irF is, bit for bit, what resample_kernel gives for the whole of ir44 from zero state in
 *   one final call (ft_test_resample), at Fo = 44100 ir44 itself - exactly as Mix prepares its bed.  Its length is nh;
 *   nh - offset < 1 is FT_ERR_ARG.  L = nh - offset with length = 0, else min(length, nh - offset); L > 131072 is
 *   FT_ERR_TOO_LONG: the caller chooses a length, nothing is cut silently.  f = min(fade, L); t[k] = irF[offset + k], and for
 *   k >= L - f it is multiplied once by ramp(L - 1 - k), the join's ramp with fade length f.
 *   Energy: e_b = the sum over k ascending inside block b of 256 taps of (double) t[k] (double) t[k], every product exact and
 *   every addition rounded to float64; E = the sum of the e_b, b ascending.  With normalize gn = (float)(1 / sqrt(E)), float64
 *   rounded once, and E = 0 or a non-finite E is FT_ERR_ARG after the launches; without it gn = 1.  hn[k] = t[k] gn, one
 *   float32 product.
 *   Send: with T the table of ft_mix_gains, xs[i] = x[i] T[s(i)], one float32 product, and +0.0 where s(i) = -1.
 *   Length: N = n + tl; tl = predelay + L - 1 with tail = -1, else tl = tail, and tail > predelay + L - 1 is FT_ERR_ARG.
 *   Convolution: for i in [0, N), acc = +0.0; for k = 0 .. L - 1 ascending acc = fmaf(hn[k], xs[i - predelay - k], acc), xs
 *   being +0.0 outside [0, n): one unbroken chain, no partial sums, no split over the taps with a later addition.
 *   c[i] = acc + 0.0 (a chain that ends at -0.0 gives +0.0).
 *   Sum: y[i] = T[dry] x[i] + T[wet] c[i], both products and the sum rounded to float32 on their own; x is +0.0 at i >= n,
 *   and with dry = -1 the first term is +0.0.
 *   Ceiling, with ceiling = 1: Mix's rule - pk = max |y| (a NaN is never the peak), c = 10^(-1/20); if pk > c every sample is
 *   multiplied once by sg = (float)(c / pk) (float64, rounded once), else nothing more touches a sample.  With ceiling = 0
 *   (a mix stage follows and has the ceiling) nothing more touches a sample and pk is still reported.
 *   Non-finite values: the call does not look for them.  If x[j] is not finite every y[i] with i outside
 *   [j - 1024, j + predelay + L + 1024) is still as stated; inside that range any value may stand (the kernel pads the chain
 *   with terms 0 x).  float32 subnormals are kept.
 *   It follows: a one-sample IR of 1.0 with wet = 0, dry = -1, no predelay and no regions gives y = x (a -0.0 becomes +0.0);
 *   muting every send gives y[i] = T[dry] x[i] and then tl zeros; a call repeated gives the same bits (no floating-point
 *   atomics; the peak is a max); shifting predelay by p shifts c by p.
 *   In a stereo call the room stage runs on the mono programme, before the panning: the last pan region is extended over
 *   the tail, so the wet signal is panned with the programme that excites it.
 *   Reported (ft_room_info): N, nh, L, E, gn, pk, sg (1 when not capped), capped, the IR's ft_intake_info.
 * Every argument is checked before any device work and a refused call changes nothing.  The checks, in this order: a null
 * pointer; sample_rate; n < 1; the regions (Stereo mix's region checks, a send in the pan's place); channel as the intake judges
 * it; normalize; wet; dry; send; ceiling; offset; length; fade; predelay; tail < -1 (FT_ERR_ARG each); n beyond 2^28
 * (FT_ERR_TOO_LONG); nh - offset < 1 (FT_ERR_ARG); L (FT_ERR_TOO_LONG); tail beyond predelay + L - 1 (FT_ERR_ARG); N beyond
 * 2^28 (FT_ERR_TOO_LONG); capacity < N (FT_ERR_ARG); then the IR as ft_codec_intake judges an item (an item whose rate or
 * frame count the intake refuses has no nh: the checks that need it are passed over and the intake's refusal stands).
 * Lock and stream are the codec's, as for Mix.
 * On the device: the programme and the output in the mix stage's buffers, the sent programme, t, hn, one float64 per block of
 * taps.  Launches beyond the IR's preparation: room_ir_kernel (offset, fade, block energies), room_gain_kernel (E and gn by one
 * thread, then hn), room_send_kernel (left out without regions and with rp->send = 0: the chain then reads x),
 * room_conv_kernel (the chain on v_mfma_f32_32x32x2_f32 with the sum and the peak; 2^22 outputs per launch), and
 * mix_scale_kernel when the ceiling binds. */
typedef struct ft_send_region {
    int64_t a, e;
    int32_t send, reserved;
} ft_send_region;
typedef struct ft_room_params {
    int32_t channel, normalize, wet, dry, send, ceiling;
    int64_t offset, length, fade, predelay, tail;
} ft_room_params;
typedef struct ft_room_info {
    int64_t N, nh, L;
    double E;
    float gn, pk, sg;
    int32_t capped;
    ft_intake_info ir;
} ft_room_info;
ft_status ft_codec_room(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_send_region* regions, int32_t R,
                        const ft_intake_item* ir, const ft_room_params* rp, float* y, int64_t capacity, int64_t* total,
                        ft_room_info* info);
/* Host only: L and N of a call whose IR has nh samples at the output rate.  Either output pointer may be NULL.  FT_ERR_ARG /
 * FT_ERR_TOO_LONG as ft_codec_room judges the values. */
ft_status ft_room_plan(int32_t sample_rate, int64_t n, int64_t nh, const ft_room_params* rp, int64_t* L, int64_t* N);
/* Live room.  The room stage on a stream: synthesize_long_stream and synthesize_script_stream hand out audio before the piece
 * ends.  Of Room only the ceiling - one gain from the peak of the whole piece - needs the whole piece; the convolution is
 * causal: c[i] reads xs[i - predelay - k] for k >= 0, so an output is final the moment its input sample has arrived and nothing
 * is held back.  Room, its bits and its refusals stay as they are; what this paragraph does not state is Room's.  Stated, which
 * fixes every bit of the result for finite inputs:
 *   Inputs: the programme x at the output rate Fo, float32, in pushes of any size (0 samples allowed; n is known at `final`,
 *   and n = 0 is allowed).  Each push carries its own send regions, ft_send_region {a, e, send} relative to that push:
 *   0 <= a < e <= n_push, sorted and disjoint (they may touch), a send in [0, 6000] or -1, 0 <= R <= 4096 per push; a push of 0
 *   samples takes R = 0.  A line that crosses a cut is given as two regions of equal send.  One IR item and ft_room_params as
 *   ft_codec_room takes them, with rp->ceiling = 0: a stream has no whole-piece peak, and a live mix stage behind it has the
 *   limiter (ft_codec_mix_stream_begin_bare where the stream has neither bed nor panning).
 *   begin: the response prepared as ft_codec_room prepares it - the intake launches and the resampler as Mix prepares its bed,
 *   room_ir_kernel, room_gain_kernel - and hn kept on the device for the life of the stream.  With normalize, E = 0 or a
 *   non-finite E is FT_ERR_ARG after those launches, and the stream is freed.
 *   push: with n_in the samples pushed before, a push of n samples emits exactly the outputs [n_in, n_in + n) of Room's y; a
 *   `final` push emits [n_in, n_in + n + tl), tl by Room's tail rule.  Nothing is held back.
 *   Result: the concatenated outputs are, bit for bit and whatever the cutting, the y of ft_codec_room with ceiling = 0 on the
 *   concatenated programme with every push's regions moved to the timeline (a region of a push that begins at n_in lies at
 *   [n_in + a, n_in + e)).  The chain of an output is Room's chain - the same kernel text over another source of xs - and xs
 *   outside what has been pushed is +0.0, as Room's is outside [0, n).  A stream whose programme is empty at `final` emits tl
 *   samples of +0.0.
 *   Non-finite values: Room's range, with one difference that only narrows it - an output emitted by a push earlier than the
 *   one that holds x[j] is as stated even inside [j - 1024, j).
 *   Reported (ft_room_info, by ft_codec_room_stream_info at any time and by ft_codec_room_live): nh, L, E, gn and the IR's
 *   ft_intake_info from `begin`; N = the samples emitted so far; pk = the max |y| over the pushes so far, by the integer atomicMax
 *   of Room (a NaN is never the peak); sg = 1 and capped = 0.
 * Limits and refusals.  begin: Room's checks in Room's order, without n, the regions and the capacity; a ceiling other than 0 is
 * FT_ERR_ARG where Room judges the ceiling.  push: everything is judged before any device work and a refused push leaves its
 * stream as it was.  In this order: a push after `final` (FT_ERR_STATE); n < 0 or a null x with n > 0; the regions (Room's
 * region checks over the push's n) (FT_ERR_ARG each); n_in + n + tl beyond 2^28 (FT_ERR_TOO_LONG, at the push that would cross
 * it); a capacity below what the push emits (FT_ERR_ARG).  Several room streams may be open on one context, each with its own
 * state; all device work runs on the codec's stream, under the codec's lock.
 * On the device a stream holds hn, the words its launches reduce into (E, gn, pk) and a carry of the last
 * min(n_in, predelay + L - 1) sent samples in two copies (a push reads one and writes the other), so its memory is bounded by
 * predelay + L - 1 - plus, in the context's buffers, the largest push - never by the length of the stream; the counters live on
 * the host.  Three launches per push, a launch with nothing to do left out: rooml_send_kernel (xs of the push from its own
 * regions; left out without regions and with rp->send = 0), rooml_conv_kernel (room_conv_kernel's text, a word of its staging
 * taken from the carry, from the push, or +0.0 outside both; the dry term from the push; 2^22 outputs per launch),
 * rooml_roll_kernel (the next carry from the old one and the push). */
typedef struct ft_room_stream ft_room_stream;
/* A stream of the stage: prepares the response and allocates the stream's state. */
ft_status ft_codec_room_stream_begin(ft_ctx* ctx, int32_t sample_rate, const ft_intake_item* ir, const ft_room_params* rp,
                                     ft_room_stream** out);
/* One push of n >= 0 programme samples (host; x may be NULL when n = 0) with its R regions (relative to the push; regions may be
 * NULL when R = 0); final: the programme ends with it.  The outputs are written into y (host, `capacity` samples) and their
 * count into *n_out: n, or n + tl at `final`. */
ft_status ft_codec_room_stream_push(ft_room_stream* rs, const float* x, int64_t n, const ft_send_region* regions, int32_t R,
                                    int32_t final, float* y, int64_t capacity, int64_t* n_out);
/* What the stream did so far (above: Reported). */
ft_status ft_codec_room_stream_info(ft_room_stream* rs, ft_room_info* info);
/* Frees the stream (after its context was destroyed: the host handle alone). */
void ft_codec_room_stream_end(ft_room_stream* rs);
/* The stage on a host waveform, as a stream whose only push is its last: y receives the N = n + tl samples (capacity >= N),
 * *total = N.  x may be NULL when n = 0. */
ft_status ft_codec_room_live(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_send_region* regions, int32_t R,
                             const ft_intake_item* ir, const ft_room_params* rp, float* y, int64_t capacity, int64_t* total,
                             ft_room_info* info);
/* Live mix.  The mix stage on a stream: synthesize_long_stream and synthesize_script_stream hand out audio before the piece
 * ends, and the one gain of Mix's ceiling is known only there.  Everything in Mix before the ceiling is local in time, so this
 * second stage keeps it as it is and replaces the one gain by a look-ahead limiter with the duck's own cone shape, driven by
 * the peaks of the mixed hops; it then holds back less than half a second.  It is a different operation from Mix - a gain that
 * varies in time - and Mix, its ceiling and its refusals stay as they are.  Stated, which fixes every bit of the result:
 *   Inputs: the programme x[0 .. n) at the output rate Fo, float32, arriving in pushes of any size; a push of 0 samples is
 *   allowed; n is known at `final` and n = 0 is allowed.  One bed item and ft_mix_params, both as ft_codec_mix takes them:
 *   the same fields, the same checks in the same order (n < 0 where Mix refuses n < 1).
 *   Constants: H = floor(Fo / 50); T[d] the table of ft_mix_gains; cf = (float) 10^(-1/20); limiter attack La = 5 hops and
 *   release Lr = 25 hops.
 *   Bed, timeline, activity, duck, gains: exactly as Mix states them, with N = lead + n + tail and Nh = ceil(N / H).  The bed is
 *   prepared once, at `begin` - intake, level, join with (0, 1, 0, 0), then the resampler from zero state - and stays on the
 *   device for the life of the stream; nb = 0 is FT_ERR_ARG after those launches, as in ft_codec_mix.
 *   Fades: N is not known while streaming, so Mix's N / 2 clamps go: f_in = fade_in and f_out = fade_out (a fade beyond 2^30
 *   samples, four times the longest timeline, counts as 2^30).  A sample with i < f_in gets t = t ramp_in(i); one with
 *   i >= N - f_out then gets t = t ramp_out(N - 1 - i); a sample in both ranges gets both products, in that order, each
 *   rounded on its own.  The rest of the sample rule is Mix's, so for N >= 2 max(fade_in, fade_out) the sample before the
 *   limiter, m[i], is Mix's m[i] bit for bit.
 *   Limiter: Q_h = max |m| over hop h (a NaN is never the peak; 0 for a hop of NaNs).  need_h is the smallest d in [0, 6000]
 *   with __fmul_rn(T[d], Q_h) <= cf, 6000 if there is none (T is monotone: a binary search finds it).  Nodes k = 0 .. Nh:
 *   L_k is the largest of 0, need_h (La - (h - k)) / La over h in [k, k + La - 1] and need_h (Lr - (k - 1 - h)) / Lr over h in
 *   [k - Lr, k - 1]; only hops in [0, Nh) count; integer divisions in int64.  Unlike the duck, every hop of a window counts, not
 *   the nearest alone, because need varies from hop to hop.  l_k = T[L_k].  For i = k H + j:
 *   y[i] = __fmul_rn(m[i], fmaf(__fdiv_rn((float) j, (float) H), l_k+1 - l_k, l_k)).  Both nodes of hop h sit at need_h or
 *   deeper, so |y| <= cf up to rounding; where L_k = L_k+1 = 0 the factor is exactly 1 and y = m bit for bit.  So a call whose m
 *   never exceeds cf, with N >= 2 max(fade_in, fade_out), equals ft_codec_mix bit for bit.
 *   Emission: after n_in programme samples, not final, let F = lead + n_in and W' = floor(F / H).  The activity is final for
 *   hops h < W', D_k for k <= W' - Wa; m[i] where both of its nodes are and i < E = lead + n_in + tail - fade_out (a later
 *   sample might still lie in the fade-out); Q_h for h < Wm = min(max(0, W' - Wa), floor(max(0, E) / H)); L_k for
 *   k <= Wm - La; and the outputs below max(0, Wm - La) H, which go out.  `final` fixes N, computes the rest and emits all N
 *   samples.  The stage holds back less than (Wa + La + 2) H + max(0, fade_out - tail) samples, 0.44 s at the default attack;
 *   an empty first push emits what `lead` alone makes final.
 *   Determinism: no floating-point atomics; Q_h is reduced inside the one workgroup that owns hop h; nothing depends on how the
 *   pushes were cut.
 *   Reported (ft_mix_live_info, by ft_codec_mix_live): N, nb, Nh, the active hops, the largest D_k (dmax), the largest L_k
 *   (lmax), the largest Q_h (qmax), the bed's ft_intake_info.
 * Limits and refusals: every argument is checked before any device work, in ft_codec_mix's order, and a refused call changes
 * nothing - a refused push leaves its stream as it was.  A push after `final` is FT_ERR_STATE; a capacity below what the push
 * emits (ft_mix_live_plan says how much) is FT_ERR_ARG; N beyond 2^28 is FT_ERR_TOO_LONG at the push that would cross it.
 * Several mix streams may be open on one context, each with its own state; all device work runs on the codec's stream.
 * On the device a stream holds its bed, two carries in two copies each (a push reads one and writes the other) - the programme
 * not yet mixed, below (Wa + 2) H + max(0, fade_out - tail) samples, and the m not yet emitted, at most La H - and whole arrays
 * of act, D_k, g_k, need_h and L_k, 17 bytes per 20 ms, which grow on need; the counters live on the host.  Five launches per
 * push whatever its size, a launch with nothing to do left out: mixl_hop_kernel, mixl_node_kernel, mixl_sample_kernel (m, Q_h,
 * need_h), mixl_limit_kernel, mixl_apply_kernel (y, then the roll of the carries). */
typedef struct ft_mix_live_info {
    int64_t N, nb, Nh, active;
    int32_t dmax, lmax;
    float qmax;
    int32_t reserved;
    ft_intake_info bed;
} ft_mix_live_info;
typedef struct ft_mix_stream ft_mix_stream;
/* Host only: after n_in programme samples of a stream with these values (final: its end), *n_out = the samples emitted so far
 * and *nodes = the limiter nodes that are final.  Either pointer may be NULL.  FT_ERR_ARG / FT_ERR_TOO_LONG as
 * ft_codec_mix_live judges the rate, n_in and mp. */
ft_status ft_mix_live_plan(int32_t sample_rate, const ft_mix_params* mp, int64_t n_in, int32_t final, int64_t* n_out,
                           int64_t* nodes);
/* The stage on a host waveform, as a stream whose only push is its last.  y receives the N = lead + n + tail samples
 * (capacity >= N), *total = N; duck and limit (each may be NULL) receive D_0 .. D_Nh and L_0 .. L_Nh.  x may be NULL when
 * n = 0. */
ft_status ft_codec_mix_live(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_intake_item* bed,
                            const ft_mix_params* mp, float* y, int64_t capacity, int64_t* total, int32_t* duck, int32_t* limit,
                            ft_mix_live_info* info);
/* A stream of the stage: prepares the bed and allocates the stream's state. */
ft_status ft_codec_mix_stream_begin(ft_ctx* ctx, int32_t sample_rate, const ft_intake_item* bed, const ft_mix_params* mp,
                                    ft_mix_stream** out);
/* A mono stream of the stage without a bed: the limiter alone, for a stream that has a room (Live room) and neither music nor
 * panning.  Stated as Live mix with the bed term +0.0: t = +0.0, nb = 0, nothing loops, so m[i] = s[i] + 0.0, and where the
 * programme never exceeds cf the output is x + 0.0 behind `lead` zeros; mp as ft_codec_mix_stream_begin judges it, its bed
 * fields unread, the report's bed zeroed.  Pushed by ft_codec_mix_stream_push and ended by ft_codec_mix_stream_end.
 * ft_codec_mix_stream_begin keeps refusing a null bed. */
ft_status ft_codec_mix_stream_begin_bare(ft_ctx* ctx, int32_t sample_rate, const ft_mix_params* mp, ft_mix_stream** out);
/* One push of n >= 0 programme samples (host; x may be NULL when n = 0); final: the programme ends with it.  The samples that
 * became final are written into y (host, `capacity` samples) and their count into *n_out. */
ft_status ft_codec_mix_stream_push(ft_mix_stream* ms, const float* x, int64_t n, int32_t final, float* y, int64_t capacity,
                                   int64_t* n_out);
/* Frees the stream (after its context was destroyed: the host handle alone). */
void ft_codec_mix_stream_end(ft_mix_stream* ms);
/* Live stereo mix.  The live mix stage with two channels out: a streamed dialogue with its speakers panned and its bed kept in
 * stereo.  Live mix, Stereo mix, their bits and their refusals stay as they are; what this paragraph does not state is Live
 * mix's, and what Live mix does not state is Stereo mix's.  Stated, which fixes every bit of the result:
 *   Inputs: the mono programme x at the output rate, in pushes of any size (0 samples allowed).  Each push carries its own pan
 *   regions, ft_pan_region {a, e, pan} relative to that push: 0 <= a < e <= n_push, sorted and disjoint (they may touch), pan
 *   in [-100, 100], 0 <= R <= 4096 per push; a push of 0 samples takes R = 0.  A line that crosses a cut is given as two regions
 *   of equal pan, one ending a push and one beginning the next.  q(i) is the pan of the region that holds programme sample
 *   i - lead, 0 where none does.  One bed item, or NULL (a panned stream without music); ft_mix_params with Mix's fields,
 *   checks and check order.
 *   Bed: the two sides and the pair level exactly as Stereo mix states them (the sides by mp->channel, one side prepared as
 *   Mix's bed where both name one channel, else each side from the intake and one gain for the pair), each side through the
 *   resampler from zero state.  Prepared once, at `begin`, and kept on the device for the life of the stream; nb = 0 is
 *   FT_ERR_ARG after those launches.  Without a bed t = +0.0, nb = 0 and info->bed is zeroed.
 *   Timeline, activity, D_k, g_k: Live mix's, from the mono x.
 *   Sample: s_c[i] = __fmul_rn(x[i - lead], P_c(q(i))) inside [lead, lead + n), +0.0 outside; m_c[i] is Live mix's sample rule
 *   over s_c and side c of the bed - the fades without the N / 2 clamp, every product and the sum rounded on its own.
 *   Limiter: linked across the channels, so the image does not move when one channel peaks.  Q_h = max |m_c| over both
 *   channels of hop h (a NaN is never the peak); one need_h and one L_k as Live mix states them;
 *   y[2 i + c] = __fmul_rn(m_c[i], f(i)) with Live mix's interpolated factor f, the same for both channels.
 *   Emission: Live mix's (ft_mix_live_plan), counted in frames; capacity and *n_out count frames.
 *   Determinism: no floating-point atomics; nothing - no bit and no refusal beyond the per-push limit on R - depends on how the
 *   pushes were cut, wherever a cut falls in a region: every programme sample carried into a later push keeps its pan.
 *   It follows: (a) with every pan 0 and both sides one channel y[2 i] = y[2 i + 1] = ft_codec_mix_live's y[i], with the same
 *   D_k, L_k, need_h and counts; (b) where m never exceeds cf and N >= 2 max(fade_in, fade_out) the output is
 *   ft_codec_mix_stereo's for the concatenated regions, bit for bit; (c) any cutting gives the one-shot call's bits, each push
 *   emitting ft_mix_live_plan's count; (d) |y| <= cf up to one rounding on both channels.
 *   Reported (ft_mix_live_info): as Live mix, N, nb and Nh in frames, qmax over both channels, the bed's info as Stereo mix.
 * Limits and refusals: Live mix's, in its order, with the regions of a push judged behind the rate and n: a null table with
 * R > 0, R outside [0, 4096], a region out of order or outside [0, n_push), a pan outside [-100, 100] (FT_ERR_ARG each); a
 * refused push leaves its stream as it was.  ft_codec_mix_stream_push on a stereo stream and ft_codec_mix_stream_push_stereo
 * on a mono one are FT_ERR_STATE.  ft_codec_mix_stream_end serves both kinds.
 * On the device a stereo stream holds both sides of its bed (each on a 16-byte boundary), Live mix's per-hop arrays and three
 * carries in two copies each: the mono programme not yet mixed, one pan byte (pan + 100) per carried programme sample in the
 * same layout, and the m not yet emitted, at most 2 La H floats.  Every sample buffer is laid out by the timeline index minus a
 * multiple of four, so a group of four frames that begins at a multiple of four lies on a 16-byte boundary in the push and in
 * the programme carry and on a 32-byte boundary in the staged m and the m carry.  Six launches per push whatever its size and
 * its R, a launch with nothing to do left out: mixl_hop_kernel, mixl_node_kernel, mixls_pan_kernel (the push's regions to one
 * pan byte per sample), mixls_sample_kernel (m_0, m_1, Q_h, need_h), mixl_limit_kernel, mixls_apply_kernel (y, then the roll of
 * the three carries). */
/* The stage on a host waveform, as a stereo stream whose only push is its last: y receives N = lead + n + tail interleaved
 * frames (capacity >= N frames), *total = N; duck, limit and info as ft_codec_mix_live; bed may be NULL. */
ft_status ft_codec_mix_live_stereo(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_pan_region* regions,
                                   int32_t R, const ft_intake_item* bed, const ft_mix_params* mp, float* y, int64_t capacity,
                                   int64_t* total, int32_t* duck, int32_t* limit, ft_mix_live_info* info);
/* A stereo stream of the stage: prepares the bed's sides (bed may be NULL) and allocates the stream's state. */
ft_status ft_codec_mix_stream_begin_stereo(ft_ctx* ctx, int32_t sample_rate, const ft_intake_item* bed, const ft_mix_params* mp,
                                           ft_mix_stream** out);
/* One push of n >= 0 programme samples with its R regions (relative to the push; regions may be NULL when R = 0).  The frames
 * that became final are written into y (host, 2 * capacity floats) and their count into *n_out. */
ft_status ft_codec_mix_stream_push_stereo(ft_mix_stream* ms, const float* x, int64_t n, const ft_pan_region* regions, int32_t R,
                                          int32_t final, float* y, int64_t capacity, int64_t* n_out);

/* ---- FLAC: a finished waveform packed losslessly on the device (csrc/flac_kernels.h; host arithmetic csrc/flac_plan.h).
 * The stage, stated to the bit:
 *   Inputs: x on the host, n >= 1 frames of `channels` (1 or 2) interleaved samples; fmt 0 is float32, 1 is int16 taken as it
 *   is; sample_rate any rate ft_resample_filter accepts; ft_flac_params {blocksize B in {256, 512, 1024, 2048, 4096}, reserved 0}.
 *   Quantisation (fmt 0): p = (int) trunc(min(1, max(-1, x)) 32767.0f), one float32 product; a NaN gives 0.  16 bits per sample.
 *   Stream: `fLaC`, then one STREAMINFO block with the last-block flag set (header 80 00 00 22): min blocksize = max blocksize =
 *   B (16 bits each), the real minimum and maximum frame size (24 bits each), the rate (20 bits), channels - 1 (3), 15 (5),
 *   n (36 bits), the MD5 field all zero ("not computed": the PCM never reaches the host).  Then F = ceil(n / B) frames of B
 *   samples, the last of n - (F - 1) B.
 *   Frame header: FF F8 (sync, fixed blocksize); the blocksize code 1000..1100 for 256..4096 when the frame has B samples, for a
 *   short last frame of bs samples 0110 with bs - 1 in 8 bits when bs <= 256, else 0111 with bs - 1 in 16 bits; the rate code
 *   0100 8000, 0101 16000, 0110 22050, 0111 24000, 1000 32000, 1001 44100, 1010 48000, any other rate 1101 with the rate in Hz
 *   in 16 bits; the channel assignment (4 bits); the sample-size code 100 and a 0 bit; the frame number in the format's
 *   UTF-8-style coding; the blocksize extra, then the rate extra; CRC-8 (poly 0x07, init 0) over the header so far.
 *   Channel assignment: mono 0000.  Stereo: M = (L + R) >> 1 (arithmetic shift), S = L - R (17 bits); the least total of
 *   subframe bits wins among 0001 (L, R), 1000 (L, S), 1001 (S, R) and 1010 (M, S), ties in that order.
 *   Subframe of a channel of width w (16; 17 for S), one header byte with the wasted-bits flag 0.  Candidates and their bits:
 *   CONSTANT (000000), only when all samples are equal: 8 + w.  FIXED o (001ooo) for o = 0..4 with o < bs: 8 + w o + 6 + the
 *   residual's cost.  VERBATIM (000001): 8 + w bs.  The least wins; ties go CONSTANT, FIXED by ascending o, VERBATIM.
 *   Residual: the format's fixed predictors, e_0 = s, e_o[i] = e_(o-1)[i] - e_(o-1)[i-1]; u = 2 e for e >= 0, else -2 e - 1.
 *   Coding method 00 (4-bit parameters), the escape never used.  A partition order P is allowed when P <= 8, 2^P divides bs and
 *   (bs >> P) > o; the first partition holds (bs >> P) - o residuals.  A partition of m residuals with parameter k in 0..14
 *   costs 4 + sum(u >> k) + m (k + 1); the least k-cost per partition wins, ties to the smaller k; the least total over P wins,
 *   ties to the smaller P.  The search is exhaustive: sum(u >> k) is additive over partitions, so the 15 sums are taken at the
 *   finest partitions (2^min(8, trailing zeros of bs)) and merged pairwise upward.  A residual is u >> k zero bits, a one, the
 *   k low bits of u.
 *   Frame end: zero bits to the byte, then CRC-16 (poly 0x8005, init 0, big-endian) over the whole frame.
 *   Determinism: integer arithmetic behind the one float32 product, integer atomics only: a repeated call gives the same bytes.
 *   Reported (ft_flac_info): frames F, bytes (= *total), the smallest and the largest frame, a count per subframe kind
 *   (CONSTANT, VERBATIM, FIXED 0..4), a count per channel assignment (0000, 0001, 1000, 1001, 1010).
 * Limits and refusals: every argument is checked before any device work, and a refused call changes nothing.  In this order:
 * a null pointer; fmt; channels; sample_rate; blocksize; reserved; n < 1 (FT_ERR_ARG each); n beyond 2^28 (FT_ERR_TOO_LONG);
 * capacity < ft_flac_bound (FT_ERR_ARG).  The bound is the all-VERBATIM stream with the longest frame header, which the encoder
 * cannot exceed because VERBATIM is always a candidate.
 * Four launches whatever n: flac_analyse_kernel (one workgroup per frame and signal - L, R, M, S in stereo: the cost search),
 * flac_pack_kernel (one workgroup per frame: assignment, header, a scan over the code lengths, the codes ORed into a zeroed
 * LDS image, both CRCs, the frame to a worst-case-stride slot), flac_scan_kernel (one workgroup: the frames' places, the
 * smallest and largest, the 42 leading bytes), flac_gather_kernel (the slots to the compact stream).  The host reads the
 * counters, then the `total` bytes and nothing else. */
typedef struct ft_flac_params {
    int32_t blocksize, reserved;
} ft_flac_params;
typedef struct ft_flac_info {
    int64_t frames, bytes;
    int32_t min_frame, max_frame;
    int32_t kinds[7];
    int32_t assignments[5];
} ft_flac_info;
ft_status ft_codec_flac(ft_ctx* ctx, const void* x, int32_t fmt, int64_t n, int32_t channels, int32_t sample_rate,
                        const ft_flac_params* fp, uint8_t* out, int64_t capacity, int64_t* total, ft_flac_info* info);
/* Host only: 42 + F (17 + channels) + 2 channels n bytes, F = ceil(n / blocksize); -1 for arguments ft_codec_flac refuses. */
int64_t ft_flac_bound(int64_t n, int32_t channels, int32_t blocksize);
/* Live FLAC.  The FLAC stage on a stream: the samples arrive in pushes of any size and the frames go out as they complete.
 * FLAC, its bits and its refusals stay as they are; what this paragraph does not state is FLAC's.  Stated:
 *   Stream: made for `channels` (1 or 2), fmt (0 float32, 1 int16), sample_rate and ft_flac_params {blocksize B, reserved 0},
 *   checked as ft_codec_flac checks them, in its order (a null pointer; fmt; channels; sample_rate; blocksize; reserved).
 *   Push: n >= 0 frames of `channels` interleaved samples on the host, and a `final` flag.  With the carry r in [0, B) that
 *   the pushes so far left and T = r + n, the push emits F = floor(T / B) frames, ceil(T / B) when final, numbered
 *   F_done .. F_done + F - 1, over carry || push in order; the last frame of a final push has T - (F - 1) B samples.  The
 *   rest is the new carry: r' = T - F B, 0 when final.  The output of a push is the bytes of those frames and nothing else; a
 *   push that completes no frame emits 0 bytes.  A frame depends on its own samples and its number only (FLAC).
 *   Quantisation: FLAC's rule, applied when a sample enters the staging buffer; the carry holds quantised int16 samples
 *   whatever fmt is, and the frame kernels always read int16.
 *   Head: ft_codec_flac_stream_head writes FLAC's 42 leading bytes from what is known: before the final push with the
 *   smallest frame, the largest frame and n all 0, which the format reads as "unknown"; after it with the real n_in and the
 *   real smallest and largest frame.  Min and max blocksize are B in both.
 *   It follows: (1) for any cutting of an input into pushes, empty ones included, the concatenated outputs are
 *   ft_codec_flac(whole)[42:], byte for byte; (2) the final head is ft_codec_flac(whole)[:42]; (3) every push emits exactly
 *   ft_flac_stream_plan's frames within its byte bound, and the final ft_flac_info is the one-shot call's; (4) streams
 *   interleaved on one context, with one-shot calls between their pushes, do not change one another's bytes.
 *   Reported (ft_flac_info, ft_codec_flac_stream_info): the stream so far - frames, bytes (the 42 counted), the smallest and
 *   the largest frame (0 before the first), the counts per subframe kind and per channel assignment.
 * Limits and refusals of a push, in this order, before any device work; a refused push leaves the stream exactly as it was:
 * a null pointer (fs, out, n_bytes); n < 0, or x null with n > 0 (FT_ERR_ARG each); a push after the final one
 * (FT_ERR_STATE); n > 2^28, or n_in + n > 2^36 - 1, the STREAMINFO field (FT_ERR_TOO_LONG); capacity below
 * ft_flac_stream_plan's bound (FT_ERR_ARG).
 * On the device a stream holds its carry - fewer than B frames of quantised int16 samples, interleaved - in two copies that
 * alternate: a push reads one and writes the other, so the roll never overlaps.  Its device memory does not grow.  On the
 * host it keeps n_in, F_done, the running smallest and largest frame and the counts.  The staging and frame buffers are the
 * context's own, used under the codec state's mutex, so any number of streams and one-shot calls on a context may interleave.
 * Five launches per push whatever its size: flacl_stage_kernel (carry || push quantised into the int16 staging buffer, and
 * what no frame takes into the other carry copy), then FLAC's four on the staging buffer with the frame-number base F_done.
 * The frames come back from behind the 42-byte place the scan kernel fills.  A push that completes no frame is the staging
 * launch alone, and nothing is copied back. */
typedef struct ft_flac_stream ft_flac_stream;
ft_status ft_codec_flac_stream_begin(ft_ctx* ctx, int32_t channels, int32_t fmt, int32_t sample_rate, const ft_flac_params* fp,
                                     ft_flac_stream** out);
/* One push: the bytes of the frames it completes into out (host, `capacity` bytes), their count into *n_bytes. */
ft_status ft_codec_flac_stream_push(ft_flac_stream* fs, const void* x, int64_t n, int32_t final, uint8_t* out, int64_t capacity,
                                    int64_t* n_bytes);
ft_status ft_codec_flac_stream_head(ft_flac_stream* fs, uint8_t out[42]);
ft_status ft_codec_flac_stream_info(ft_flac_stream* fs, ft_flac_info* info);
/* Frees the stream (after its context was destroyed: the host handle alone). */
void ft_codec_flac_stream_end(ft_flac_stream* fs);
/* Host only: what a push of n frames emits on a stream that has taken `before` frames: *frames, and *bytes, the bound of
 * their bytes - the all-VERBATIM frames with the longest headers, as ft_flac_bound without the 42.  Either pointer may be NULL.
 * FT_ERR_ARG for a blocksize or channels the stage refuses, before < 0 or n < 0; FT_ERR_TOO_LONG beyond the push's limits. */
ft_status ft_flac_stream_plan(int32_t blocksize, int32_t channels, int64_t before, int64_t n, int32_t final, int64_t* frames,
                              int64_t* bytes);

ft_status ft_sync(ft_ctx* ctx);
/* State of the persistent frame engine (csrc/frame_engine.h), the batch-1 form of the decode step
 * (fish_tts/models/inference.py:83-155 as two launches of one workgroup per CU instead of ~325 launches).
 * flags bit 0: the slow stack runs on it, bit 1: the fast codebook loop runs on it (0 = this context takes the launch
 * path: other widths, f32 precision, FT_NO_ENGINE set, another context of the process owns the device's engine, or the
 * engine was turned off after repeated time-outs).  aborted = hand-off time-outs so far: each one was recovered inside
 * the call that hit it (control words and hand-off buffers cleared, the affected frames redone on the launch path, so
 * the call still returns the frames the launch path yields); after two the context stops using the engine.
 * where = the phase that gave up first in the last such event.  Any pointer may be NULL. */
ft_status ft_ar_engine_state(ft_ctx* ctx, int32_t* flags, int32_t* aborted, int32_t* where);
/* One line of text: which path the batch-1 decode frames of this context take and why (for the host's log). */
const char* ft_ar_frame_path(const ft_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
