// libfishtts_hip.so: context, weight ingestion, the AR prefill/decode drivers (hipGraph-captured
// frame step) and the C ABI declared in include/fishtts_hip.h.
#include "engine.h"
#include "ar_kernels.h"
#include "frame_engine.h"
#include "wide_kernels.h"
#include "gemm_kernels.h"
#include "codec_kernels.h"
#include "stage_kernels.h"

#include <math.h>

#include <algorithm>
#include <mutex>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace ft;

static std::string g_create_err;
static void eng_release(ft_ctx* ctx);

ft_status ft_fail(ft_ctx* ctx, ft_status code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_err = msg;
    return code;
}

// ------------------------------------------------------------------------------------------ utils
template <typename S, typename D>
__global__ void convert_kernel(const S* s, D* d, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        st_elem(d, (size_t)i, ld_elem(s, (size_t)i));
}
template <typename T>
__global__ void interleave_rows_kernel(const T* a, const T* b, T* o, int64_t rows, int64_t K) {
    const int64_t n = rows * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / K, k = i % K;
        o[(2 * r) * K + k] = a[i];
        o[(2 * r + 1) * K + k] = b[i];
    }
}

template <typename T>
static ft_status dmalloc(ft_ctx* ctx, T** p, size_t n) {
    void* q = nullptr;
    const size_t bytes = n * sizeof(T) ? n * sizeof(T) : 16;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    hipMemset(q, 0, bytes);
    *p = (T*)q;
    return FT_OK;
}
#define FT_TRY(x) do { ft_status s_ = (x); if (s_ != FT_OK) return s_; } while (0)

// ------------------------------------------------------------------------------------------ names
void ft_expect(ft_ctx* ctx, const std::string& name, std::vector<int64_t> shape, int dtype) {
    FtTensor t;
    t.shape = std::move(shape);
    t.dtype = dtype;
    ctx->expected[name] = t;
}

static void ar_expected(ft_ctx* ctx) {
    const ft_ar_config& c = ctx->c;
    const int dt = c.dtype;
    ft_expect(ctx, "embeddings.weight", {c.vocab_size, c.dim}, dt);
    ft_expect(ctx, "codebook_embeddings.weight", {(int64_t)c.codebook_size * c.num_codebooks, c.dim}, dt);
    auto block = [&](const std::string& p, int dim, int nh, int nkv, int hd, int ffn, int qkvb, int ob, int qkn) {
        const int64_t tot = (int64_t)(nh + 2 * nkv) * hd;
        ft_expect(ctx, p + ".attention.wqkv.weight", {tot, dim}, dt);
        if (qkvb) ft_expect(ctx, p + ".attention.wqkv.bias", {tot}, dt);
        ft_expect(ctx, p + ".attention.wo.weight", {dim, (int64_t)nh * hd}, dt);
        if (ob) ft_expect(ctx, p + ".attention.wo.bias", {dim}, dt);
        if (qkn) {
            ft_expect(ctx, p + ".attention.q_norm.weight", {hd}, dt);
            ft_expect(ctx, p + ".attention.k_norm.weight", {hd}, dt);
        }
        ft_expect(ctx, p + ".feed_forward.w1.weight", {ffn, dim}, dt);
        ft_expect(ctx, p + ".feed_forward.w3.weight", {ffn, dim}, dt);
        ft_expect(ctx, p + ".feed_forward.w2.weight", {dim, ffn}, dt);
        ft_expect(ctx, p + ".ffn_norm.weight", {dim}, dt);
        ft_expect(ctx, p + ".attention_norm.weight", {dim}, dt);
    };
    for (int i = 0; i < c.n_layer; ++i)
        block("layers." + std::to_string(i), c.dim, c.n_head, c.n_local_heads, c.head_dim, c.intermediate_size,
              c.attention_qkv_bias, c.attention_o_bias, c.attention_qk_norm);
    ft_expect(ctx, "norm.weight", {c.dim}, dt);
    if (!c.tie_word_embeddings) ft_expect(ctx, "output.weight", {c.vocab_size, c.dim}, dt);
    if (c.fast_dim != c.dim) {
        ft_expect(ctx, "fast_project_in.weight", {c.fast_dim, c.dim}, dt);
        ft_expect(ctx, "fast_project_in.bias", {c.fast_dim}, dt);
    }
    ft_expect(ctx, "fast_embeddings.weight", {c.codebook_size, c.fast_dim}, dt);
    for (int i = 0; i < c.n_fast_layer; ++i)
        block("fast_layers." + std::to_string(i), c.fast_dim, c.fast_n_head, c.fast_n_local_heads, c.fast_head_dim,
              c.fast_intermediate_size, c.fast_attention_qkv_bias, c.fast_attention_o_bias,
              c.fast_attention_qk_norm);
    ft_expect(ctx, "fast_norm.weight", {c.fast_dim}, dt);
    ft_expect(ctx, "fast_output.weight", {c.codebook_size, c.fast_dim}, dt);
    // RoPE tables exactly as the reference stores them (llama.py:594-603): bf16-rounded cos/sin,
    // supplied by the host so the table is bit-identical; kept as f32 in HBM.
    ft_expect(ctx, "rope.slow", {c.max_seq_len, c.head_dim / 2, 2}, FT_F32);
    ft_expect(ctx, "rope.fast", {c.num_codebooks, c.fast_head_dim / 2, 2}, FT_F32);
}

// ------------------------------------------------------------------------------------------ create
static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

static ft_status ar_validate(ft_ctx* ctx) {
    const ft_ar_config& c = ctx->c;
    auto bad = [&](const char* m) { return ft_fail(ctx, FT_ERR_UNSUPPORTED, m); };
    if (c.dtype != FT_BF16 && c.dtype != FT_F32 && c.dtype != FT_F16) return bad("dtype must be FT_BF16, FT_F16 or FT_F32");
    if (c.dim % 8 || c.fast_dim % 8 || c.intermediate_size % 8 || c.fast_intermediate_size % 8)
        return bad("dim / intermediate sizes must be multiples of 8");
    if (!pow2(c.head_dim) || c.head_dim < 8 || c.head_dim > 128) return bad("head_dim must be a power of two in [8,128]");
    if (!pow2(c.fast_head_dim) || c.fast_head_dim < 16 || c.fast_head_dim > 128)
        return bad("fast_head_dim must be a power of two in [16,128]");
    if (c.n_head % c.n_local_heads || c.fast_n_head % c.fast_n_local_heads) return bad("n_head % n_local_heads != 0");
    const int G = c.n_head / c.n_local_heads;
    if (G != 1 && G != 2 && G != 4 && G != 8) return bad("n_head / n_local_heads must be 1, 2, 4 or 8");
    if (c.num_codebooks < 1 || c.num_codebooks > FAST_MAXCB) return bad("num_codebooks must be in [1,16]");
    if (c.max_batch < 1 || c.max_batch > 256) return bad("max_batch must be in [1,256]");
    if (c.max_new_tokens < 1) return bad("max_new_tokens must be >= 1");
    if (c.vocab_size <= c.semantic_end_id || c.semantic_begin_id > c.semantic_end_id) return bad("bad semantic id range");
    return FT_OK;
}

static ft_status ar_alloc(ft_ctx* ctx) {
    const ft_ar_config& c = ctx->c;
    const size_t M = c.max_batch;
    ctx->esz = c.dtype == FT_F32 ? 4 : 2;
    ctx->n_slots = c.max_seq_len + ((8 - c.max_seq_len % 8) % 8);  // llama.py:387
    const char* ns = getenv("FT_ATTN_NSPLIT");
    ctx->nsplit = ns ? atoi(ns) : (ctx->n_slots > 512 ? 8 : 1);
    ctx->nsplit_fixed = ns != nullptr;
    ctx->nsplit_max = ctx->nsplit_fixed ? ctx->nsplit : (ctx->n_slots > 3072 ? 32 : ctx->n_slots > 768 ? 16 : ctx->nsplit);
    // One kv head per XCD (frame_engine.h, XL): 8 kv heads of 2 x 128-wide query heads on a chip of 8 XCDs x 32 CUs split every
    // head's cached positions 32 ways - one split per CU of the head's XCD - at every context length.  The split count is a
    // property of the shapes and the chip, not of the frame path: launches and engine then sum in the same order.
    // (Measured and not kept: short contexts walked UNSPLIT by every CU of the XCD for itself - no partials, no merge: 704 us
    // per slow-stack launch at 150 positions and 825 at 260 against 589 for the 32-way split; a 16-position step of the walk
    // costs ~0.45 us - two exact exponentials per head and step - and 10-17 of them sit on every layer's path.)
    {
        hipDeviceProp_t prop;
        ctx->xl_shape = !ns && !getenv("FT_NO_XL") && c.n_local_heads == 8 && c.n_head == 16 && c.head_dim == 128 &&
                        hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount == 256;
        if (ctx->xl_shape) { ctx->nsplit = ctx->nsplit_max = 32; ctx->nsplit_fixed = true; }
    }
    if (ctx->nsplit < 1) ctx->nsplit = 1;
    if (ctx->nsplit > 32) ctx->nsplit = 32;
    ctx->nsplit_max = std::max(1, std::min(32, std::max(ctx->nsplit_max, ctx->nsplit)));
    ctx->cap = c.max_new_tokens + 24;
    ctx->hid_in_xo.assign(M, 0);
    ctx->fastV = c.codebook_size < 1024 ? c.codebook_size : 1024;  // inference.py:134
    const size_t qkvN = (size_t)(c.n_head + 2 * c.n_local_heads) * c.head_dim;
    const size_t fqkvN = (size_t)(c.fast_n_head + 2 * c.fast_n_local_heads) * c.fast_head_dim;
    FT_TRY(dmalloc(ctx, &ctx->x, M * c.dim));
    FT_TRY(dmalloc(ctx, &ctx->qkv, M * qkvN));
    ctx->y_ld = std::max(c.n_head * c.head_dim, c.fast_n_head * c.fast_head_dim);
    FT_TRY(dmalloc(ctx, &ctx->y, M * (size_t)ctx->y_ld));
    FT_TRY(dmalloc(ctx, &ctx->g, M * c.intermediate_size));
    FT_TRY(dmalloc(ctx, &ctx->logits, M * c.vocab_size));
    if (c.fast_dim != c.dim) FT_TRY(dmalloc(ctx, &ctx->hid, M * c.fast_dim));
    else ctx->hid = ctx->x;
    FT_TRY(dmalloc(ctx, &ctx->femb, M * c.fast_dim));
    FT_TRY(dmalloc(ctx, &ctx->xf, M * c.fast_dim));
    FT_TRY(dmalloc(ctx, &ctx->qkvf, 2 * ((M + 15) / 16 * 16) * fqkvN));   // 2 x: the paired codebook pass of wide batches (positions 0 and 1 as 2 M rows)
    FT_TRY(dmalloc(ctx, &ctx->gf, M * c.fast_intermediate_size));
    FT_TRY(dmalloc(ctx, &ctx->flog, M * ctx->fastV));
    FT_TRY(dmalloc(ctx, &ctx->part_o, M * c.n_head * ctx->nsplit_max * c.head_dim));
    FT_TRY(dmalloc(ctx, &ctx->part_ml, M * c.n_head * ctx->nsplit_max * 2));
    ctx->cache_m_stride = (size_t)c.n_local_heads * ctx->n_slots * c.head_dim;
    ctx->fcache_m_stride = (size_t)c.fast_n_local_heads * c.num_codebooks * c.fast_head_dim;
    ctx->layers.resize(c.n_layer);
    ctx->flayers.resize(c.n_fast_layer);
    for (auto& l : ctx->layers) {
        FT_TRY(dmalloc(ctx, (char**)&l.kc, M * ctx->cache_m_stride * ctx->esz));
        FT_TRY(dmalloc(ctx, (char**)&l.vc, M * ctx->cache_m_stride * ctx->esz));
    }
    for (auto& l : ctx->flayers) {
        FT_TRY(dmalloc(ctx, (char**)&l.kc, M * ctx->fcache_m_stride * ctx->esz));
        FT_TRY(dmalloc(ctx, (char**)&l.vc, M * ctx->fcache_m_stride * ctx->esz));
    }
    const size_t R = c.num_codebooks + 1;
    FT_TRY(dmalloc(ctx, &ctx->d_pos, M));
    FT_TRY(dmalloc(ctx, &ctx->d_tok, M * R));
    FT_TRY(dmalloc(ctx, &ctx->d_tokn, M * R));
    FT_TRY(dmalloc(ctx, &ctx->d_seq, M * R * ctx->cap));
    FT_TRY(dmalloc(ctx, &ctx->d_nf, M));
    FT_TRY(dmalloc(ctx, &ctx->d_done, M));
    FT_TRY(dmalloc(ctx, &ctx->d_prompt, R * (size_t)c.max_seq_len));
    FT_TRY(dmalloc(ctx, &ctx->d_ctl, M));
    ctx->prefill_gemm_mode = getenv("FT_PREFILL_GEMM") ? atoi(getenv("FT_PREFILL_GEMM")) : 2;
    ctx->prefill_v0 = getenv("FT_PREFILL_V0") != nullptr || c.dtype != FT_BF16 || c.dim % 32 || (c.n_head * c.head_dim) % 32 ||
                      c.intermediate_size % 32;
    if (!ctx->prefill_v0) {
        const size_t S = c.max_seq_len;
        FT_TRY(dmalloc(ctx, &ctx->pf_x, S * c.dim));
        FT_TRY(dmalloc(ctx, &ctx->pf_qkv, S * qkvN));
        FT_TRY(dmalloc(ctx, &ctx->pf_y, S * c.n_head * c.head_dim));
        FT_TRY(dmalloc(ctx, &ctx->pf_xn, S * c.dim));
        FT_TRY(dmalloc(ctx, &ctx->pf_ybf, S * c.n_head * c.head_dim));
        FT_TRY(dmalloc(ctx, &ctx->pf_g, S * c.intermediate_size));
        FT_TRY(dmalloc(ctx, &ctx->pf_qbf, S * c.n_head * c.head_dim));
        FT_TRY(dmalloc(ctx, &ctx->pf_seqs, M));
        FT_TRY(dmalloc(ctx, &ctx->pf_rows, S));
    }
    if (c.dtype == FT_F16 || !ctx->prefill_v0) {
        // wide lock-step batches (wide_kernels.h): no fast-layer f32 bias copies exist; every contraction width must be one
        // the kernel is instantiated for, every output width a whole number of its tiles
        // (both 16-bit types; the pf_* prompt buffers above are bf16 only: ft_ar_prefill_slow_many)
        const int HD = c.n_head * c.head_dim, HDf = c.fast_n_head * c.fast_head_dim;
        ctx->wide_ok = !getenv("FT_NO_WIDE") && !c.fast_attention_qkv_bias && !c.fast_attention_o_bias && c.fast_dim == c.dim &&
                       wide_k_ok(c.dim) && wide_k_ok(HD) && wide_k_ok(c.intermediate_size) && wide_k_ok(HDf) && wide_k_ok(c.fast_intermediate_size) &&
                       qkvN % 32 == 0 && fqkvN % 32 == 0 && c.intermediate_size % 16 == 0 && c.fast_intermediate_size % 16 == 0 &&
                       c.dim % 16 == 0 && c.vocab_size % 32 == 0 && ctx->fastV % 16 == 0;
        if (ctx->wide_ok) {
            // rows [0, xo_pair) = the batch, rows [xo_pair, 2 xo_pair) = the same utterances at codebook position 1 in the
            // paired first pass of the codebook loop
            ctx->xo_pair = (int)((M + 15) / 16 * 16);
            ctx->no_pair = getenv("FT_NO_PAIR") != nullptr;
            ctx->no_attn_wide = getenv("FT_NO_ATTN_WIDE") != nullptr;
            ctx->no_head_stream = getenv("FT_NO_HEAD_STREAM") != nullptr;
            ctx->xo_ldm = 2 * ctx->xo_pair;
            const size_t P = ctx->xo_ldm;
            FT_TRY(dmalloc(ctx, &ctx->xo_x, P * c.dim));
            FT_TRY(dmalloc(ctx, &ctx->xo_xf, P * c.fast_dim));
            FT_TRY(dmalloc(ctx, &ctx->xo_femb, P * c.fast_dim));
            FT_TRY(dmalloc(ctx, &ctx->xo_y, P * (size_t)std::max(HD, HDf)));
            FT_TRY(dmalloc(ctx, &ctx->xo_g, P * (size_t)std::max(c.intermediate_size, c.fast_intermediate_size)));
        }
    }
    const size_t nchunk = ((size_t)c.vocab_size + 1023) / 1024;
    FT_TRY(dmalloc(ctx, &ctx->samp_cut, M));
    FT_TRY(dmalloc(ctx, &ctx->samp_chunk_cnt, M * nchunk));
    FT_TRY(dmalloc(ctx, &ctx->samp_part_score, M * nchunk));
    FT_TRY(dmalloc(ctx, &ctx->samp_part_idx, M * nchunk));
    FT_HIP(ctx, hipHostMalloc((void**)&ctx->h_pin, (3 * M + 8) * sizeof(int), hipHostMallocDefault));
    return FT_OK;
}

extern "C" ft_status ft_create(const ft_ar_config* ar, const ft_codec_config* codec, int32_t device, ft_ctx** out) {
    if (!out || (!ar && !codec)) return ft_fail(nullptr, FT_ERR_ARG, "ft_create: need a config and an out pointer");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return ft_fail(nullptr, FT_ERR_HIP, "ft_create: no HIP device visible (the MI355X path has no CPU fallback)");
    if (device < 0 || device >= ndev) return ft_fail(nullptr, FT_ERR_ARG, "ft_create: bad device index");
    ft_ctx* ctx = new ft_ctx();
    ctx->device = device;
    ft_status st = FT_OK;
    do {
        if (hipSetDevice(device) != hipSuccess) { st = ft_fail(ctx, FT_ERR_HIP, "hipSetDevice failed"); break; }
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            st = ft_fail(ctx, FT_ERR_HIP, "hipStreamCreate failed"); break;
        }
        if (ar) {
            ctx->c = *ar;
            ctx->has_ar = true;
            if ((st = ar_validate(ctx)) != FT_OK) break;
            if ((st = ar_alloc(ctx)) != FT_OK) break;
            ar_expected(ctx);
        }
        if (codec) {
            ctx->cc = *codec;
            ctx->has_codec = true;
            if ((st = codec_create(ctx)) != FT_OK) break;
            codec_expected(ctx);
        }
    } while (0);
    if (st != FT_OK) {
        g_create_err = ctx->err;
        ft_destroy(ctx);
        return st;
    }
    *out = ctx;
    return FT_OK;
}

extern "C" void ft_destroy(ft_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    for (auto& kv : ctx->graphs) hipGraphExecDestroy(kv.second);
    for (auto& kv : ctx->expected) if (kv.second.p) hipFree(kv.second.p);
    for (auto& l : ctx->layers) { hipFree(l.kc); hipFree(l.vc); if (l.w13) hipFree(l.w13); }
    for (auto& l : ctx->flayers) { hipFree(l.kc); hipFree(l.vc); if (l.w13) hipFree(l.w13); }
    float* bufs[] = {ctx->x, ctx->qkv, ctx->y, ctx->g, ctx->logits, ctx->femb, ctx->xf, ctx->qkvf, ctx->gf,
                     ctx->flog, ctx->part_o, ctx->part_ml, ctx->noise};
    for (float* b : bufs) if (b) hipFree(b);
    if (ctx->hid && ctx->hid != ctx->x) hipFree(ctx->hid);
    int* ibufs[] = {ctx->d_pos, ctx->d_tok, ctx->d_tokn, ctx->d_seq, ctx->d_nf, ctx->d_done, ctx->d_prompt};
    for (int* b : ibufs) if (b) hipFree(b);
    if (ctx->d_ctl) hipFree(ctx->d_ctl);
    if (ctx->wide_qkv0_tab) hipFree(ctx->wide_qkv0_tab);
    { void* pf[] = {ctx->pf_x, ctx->pf_qkv, ctx->pf_y, ctx->pf_xn, ctx->pf_ybf, ctx->pf_g, ctx->xo_x, ctx->xo_xf, ctx->xo_femb, ctx->xo_y, ctx->xo_g, ctx->pf_qbf}; for (void* q : pf) if (q) hipFree(q); }
    for (auto& l : ctx->layers) { if (l.bqkv_f32) hipFree(l.bqkv_f32); if (l.bo_f32) hipFree(l.bo_f32); }
    if (ctx->samp_cut) hipFree(ctx->samp_cut);
    if (ctx->samp_chunk_cnt) hipFree(ctx->samp_chunk_cnt);
    if (ctx->samp_part_score) hipFree(ctx->samp_part_score);
    if (ctx->samp_part_idx) hipFree(ctx->samp_part_idx);
    eng_release(ctx);
    if (ctx->h_pin) hipHostFree(ctx->h_pin);
    for (auto e : ctx->prof_ev) hipEventDestroy(e);
    codec_destroy(ctx);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" const char* ft_last_error(const ft_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

extern "C" ft_status ft_sync(ft_ctx* ctx) {
    if (!ctx) return FT_ERR_ARG;
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ weights
extern "C" ft_status ft_load_weight(ft_ctx* ctx, const char* name, const void* src, int32_t src_dtype,
                                    const int64_t* shape, int32_t ndim) {
    if (!ctx || !name || !src || !shape) return ft_fail(ctx, FT_ERR_ARG, "ft_load_weight: null argument");
    if (ctx->finalized) return ft_fail(ctx, FT_ERR_STATE, "ft_load_weight: weights already finalized");
    auto it = ctx->expected.find(name);
    if (it == ctx->expected.end()) return ft_fail(ctx, FT_ERR_ARG, std::string("unknown weight name: ") + name);
    FtTensor& t = it->second;
    if ((int)t.shape.size() != ndim) return ft_fail(ctx, FT_ERR_ARG, std::string("rank mismatch for ") + name);
    for (int i = 0; i < ndim; ++i)
        if (t.shape[i] != shape[i]) {
            char buf[256];
            snprintf(buf, sizeof buf, "shape mismatch for %s: dim %d is %lld, expected %lld", name, i,
                     (long long)shape[i], (long long)t.shape[i]);
            return ft_fail(ctx, FT_ERR_ARG, buf);
        }
    if (src_dtype != FT_F32 && src_dtype != FT_BF16 && src_dtype != FT_F16)
        return ft_fail(ctx, FT_ERR_ARG, "src_dtype must be FT_F32, FT_BF16 or FT_F16");
    FT_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = t.numel();
    const size_t ssz = src_dtype == FT_F32 ? 4 : 2, dsz = t.dtype == FT_F32 ? 4 : 2;
    if (!t.p) FT_HIP(ctx, hipMalloc(&t.p, (size_t)n * dsz + 64));
    if (src_dtype == t.dtype) {
        FT_HIP(ctx, hipMemcpy(t.p, src, (size_t)n * dsz, hipMemcpyDefault));
        return FT_OK;
    }
    void* stage = nullptr;
    FT_HIP(ctx, hipMalloc(&stage, (size_t)n * ssz));
    hipError_t e = hipMemcpy(stage, src, (size_t)n * ssz, hipMemcpyDefault);
    if (e == hipSuccess) {
        const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        auto to = [&](auto* sp) {
            if (t.dtype == FT_F32) convert_kernel<<<blocks, 256, 0, ctx->stream>>>(sp, (float*)t.p, n);
            else if (t.dtype == FT_BF16) convert_kernel<<<blocks, 256, 0, ctx->stream>>>(sp, (bf16_t*)t.p, n);
            else convert_kernel<<<blocks, 256, 0, ctx->stream>>>(sp, (f16_t*)t.p, n);
        };
        if (src_dtype == FT_F32) to((const float*)stage);
        else if (src_dtype == FT_BF16) to((const bf16_t*)stage);
        else to((const f16_t*)stage);
        e = hipStreamSynchronize(ctx->stream);
    }
    hipFree(stage);
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("ft_load_weight copy: ") + hipGetErrorString(e));
    return FT_OK;
}

static void* wp(ft_ctx* ctx, const std::string& n) {
    auto it = ctx->expected.find(n);
    return it == ctx->expected.end() ? nullptr : it->second.p;
}

static ft_status eng_setup(ft_ctx* ctx);
static ft_status wide_qkv0_build(ft_ctx* ctx);

static ft_status ar_finalize(ft_ctx* ctx) {
    const ft_ar_config& c = ctx->c;
    ctx->emb = wp(ctx, "embeddings.weight");
    ctx->cb_emb = wp(ctx, "codebook_embeddings.weight");
    ctx->norm = wp(ctx, "norm.weight");
    ctx->head = c.tie_word_embeddings ? ctx->emb : wp(ctx, "output.weight");
    ctx->fproj_w = wp(ctx, "fast_project_in.weight");
    ctx->fproj_b = wp(ctx, "fast_project_in.bias");
    ctx->fast_emb = wp(ctx, "fast_embeddings.weight");
    ctx->fast_norm = wp(ctx, "fast_norm.weight");
    ctx->fast_out = wp(ctx, "fast_output.weight");
    ctx->rope = (float*)wp(ctx, "rope.slow");
    ctx->frope = (float*)wp(ctx, "rope.fast");
    auto fill = [&](std::vector<FtLayer>& ls, const char* pre, int ffn, int dim) -> ft_status {
        for (size_t i = 0; i < ls.size(); ++i) {
            const std::string p = std::string(pre) + std::to_string(i);
            FtLayer& l = ls[i];
            l.attn_norm = wp(ctx, p + ".attention_norm.weight");
            l.wqkv = wp(ctx, p + ".attention.wqkv.weight");
            l.bqkv = wp(ctx, p + ".attention.wqkv.bias");
            l.qn = wp(ctx, p + ".attention.q_norm.weight");
            l.kn = wp(ctx, p + ".attention.k_norm.weight");
            l.wo = wp(ctx, p + ".attention.wo.weight");
            l.bo = wp(ctx, p + ".attention.wo.bias");
            l.ffn_norm = wp(ctx, p + ".ffn_norm.weight");
            l.w2 = wp(ctx, p + ".feed_forward.w2.weight");
            // w1/w3 rows interleaved so one wave owns a (gate, up) pair (SwiGLU epilogue)
            FtTensor& w1 = ctx->expected[p + ".feed_forward.w1.weight"];
            FtTensor& w3 = ctx->expected[p + ".feed_forward.w3.weight"];
            FT_HIP(ctx, hipMalloc(&l.w13, (size_t)2 * ffn * dim * ctx->esz));
            const int64_t n = (int64_t)ffn * dim;
            const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
            if (ctx->esz == 2)
                interleave_rows_kernel<bf16_t><<<blocks, 256, 0, ctx->stream>>>((bf16_t*)w1.p, (bf16_t*)w3.p, (bf16_t*)l.w13, ffn, dim);
            else
                interleave_rows_kernel<float><<<blocks, 256, 0, ctx->stream>>>((float*)w1.p, (float*)w3.p, (float*)l.w13, ffn, dim);
            FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
            hipFree(w1.p); w1.p = nullptr;
            hipFree(w3.p); w3.p = nullptr;
        }
        return FT_OK;
    };
    FT_TRY(fill(ctx->layers, "layers.", c.intermediate_size, c.dim));
    if (!ctx->prefill_v0 || ctx->wide_ok) {      // f32 bias copies of the MFMA epilogues (prompt pass: bf16; wide batches: both 16-bit types)
        const int qkvN = (c.n_head + 2 * c.n_local_heads) * c.head_dim;
        auto to_f32 = [&](const void* b, float* o, int n) {
            if (c.dtype == FT_F16) convert_kernel<f16_t, float><<<(n + 255) / 256, 256, 0, ctx->stream>>>((const f16_t*)b, o, n);
            else convert_kernel<bf16_t, float><<<(n + 255) / 256, 256, 0, ctx->stream>>>((const bf16_t*)b, o, n);
        };
        for (auto& l : ctx->layers) {
            if (l.bqkv) {
                FT_HIP(ctx, hipMalloc((void**)&l.bqkv_f32, qkvN * sizeof(float)));
                to_f32(l.bqkv, l.bqkv_f32, qkvN);
            }
            if (l.bo) {
                FT_HIP(ctx, hipMalloc((void**)&l.bo_f32, c.dim * sizeof(float)));
                to_f32(l.bo, l.bo_f32, c.dim);
            }
        }
        FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    FT_TRY(fill(ctx->flayers, "fast_layers.", c.fast_intermediate_size, c.fast_dim));
    FT_TRY(eng_setup(ctx));
    FT_TRY(wide_qkv0_build(ctx));
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ frame engine (host side)
// The engine is instantiated for a short list of shape classes (eng_slow_shapes / eng_fast_shapes below: openaudio-s1-mini's
// widths, ffn 4096, four kv heads; bf16; any depth); every other configuration keeps the launch path.  It needs every workgroup resident at once:
// one per CU, sized by the device's CU count - so only ONE context per device and process may run it (two would each
// hold part of the CUs and time each other out), and nothing in here is fatal: whatever fails leaves the launch path.
constexpr int ENG_MAX_STRIKES = 2;      // hand-off time-outs after which a context stops using the engine
static std::mutex g_eng_mu;
static std::map<int, ft_ctx*> g_eng_owner;      // device -> the context whose engine runs there

static void eng_release(ft_ctx* ctx) {
    void* eb[] = {ctx->eng_layers, ctx->eng_flayers, ctx->eng_gx /* pool: gxb, gg, gy, gqkv live in it */,
                  ctx->eng_gpart, ctx->eng_fast_g, ctx->eng_ctl, ctx->eng_qkv0_tab};
    for (void* q : eb) if (q) hipFree(q);
    ctx->eng_layers = ctx->eng_flayers = nullptr;
    ctx->eng_gx = ctx->eng_gqkv = ctx->eng_gy = ctx->eng_gxb = ctx->eng_gg = ctx->eng_fast_g = ctx->eng_ctl = nullptr;
    ctx->eng_gpart = nullptr;
    ctx->eng_qkv0_tab = nullptr;
    ctx->eng_on = ctx->eng_fast_on = false;
    if (ctx->eng_owner) {
        std::lock_guard<std::mutex> lk(g_eng_mu);
        auto it = g_eng_owner.find(ctx->device);
        if (it != g_eng_owner.end() && it->second == ctx) g_eng_owner.erase(it);
        ctx->eng_owner = false;
    }
}

// One 512-thread workgroup of `fn` with `lds` bytes of dynamic LDS on one CU: computed from the kernel's own attributes -
// waves per SIMD = 512 registers / the wave's (gfx950: one 512-entry file per SIMD lane, allocated in steps of 8), four SIMDs,
// eight waves to place.  hipOccupancyMaxActiveBlocksPerMultiprocessor is only logged: measured on this runtime it answers 0
// or 1 for the SAME kernel and attributes depending on what the process ran before (it then budgets 256 registers per lane),
// and a false 0 would silently cost the engine.  Should the answer here ever be wrong the other way, the launches time out
// and the recovery turns the engine off after ENG_MAX_STRIKES.
static bool eng_fits_cu(const void* fn, size_t lds, size_t lds_cap, const char* name, std::string& why) {
    hipFuncAttributes fa{};
    const hipError_t fe = hipFuncGetAttributes(&fa, fn);
    if (fe != hipSuccess) { (void)hipGetLastError(); why = std::string("hipFuncGetAttributes: ") + hipGetErrorString(fe); return false; }
    const int regs = std::max(fa.numRegs, 1), per_simd = 512 / (((regs + 7) / 8) * 8);
    const bool fits = per_simd * 4 >= ENG_THREADS / 64 && lds + fa.sharedSizeBytes <= lds_cap && fa.maxThreadsPerBlock >= ENG_THREADS;
    if (getenv("FT_LOG")) {
        int occ = -1;
        const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, ENG_THREADS, lds);
        if (oe != hipSuccess) (void)hipGetLastError();
        fprintf(stderr, "fish_tts_amd: %s engine kernel: %d registers (%d waves per SIMD), %zu B of LDS of %zu: %s (the occupancy query says %d)\n",
                name, fa.numRegs, per_simd, lds + fa.sharedSizeBytes, lds_cap, fits ? "fits a CU" : "does not fit a CU", occ);
    }
    if (!fits) why = std::string("a ") + name + " workgroup does not fit one CU (registers / LDS)";
    return fits;
}

// The shape classes the engine kernels are instantiated for (frame_engine.h: EngSlowShape / EngFastShape; any depth).  The
// first entries are openaudio-s1-mini's widths (config.json: llama.py:74-86); the others cover the two fields SURVEY.md could
// not verify against a real config.json - the feed-forward width and the number of kv heads (four kv heads lose the
// one-kv-head-per-XCD form of the attention and take the general split form).
typedef void (*eng_slow_fn_t)(SlowEngP);
typedef void (*eng_fast_fn_t)(FastEngP);
typedef void (*eng_qkv0_fn_t)(const bf16_t*, const bf16_t*, const bf16_t*, const bf16_t*, bf16_t*, int, int, int, float);
struct EngSlowEntry { int D, H, HKV, HDIM, F, SQ, SF, SO; eng_slow_fn_t xl, plain; };
// loop: the all-streaming form; resident: W13 pairs held in the gathering waves' registers (nullptr: nothing fits this class),
// resf pairs per gathering wave of each of up to resl layers
struct EngFastEntry { int D, H, HKV, HDIM, F, V, SQ, SF, SO; eng_fast_fn_t loop; eng_qkv0_fn_t qkv0; eng_fast_fn_t resident; int resf, resl; };
template <typename S, bool WITH_XL>
static EngSlowEntry eng_slow_entry() {
    eng_slow_fn_t xl = nullptr;
    if constexpr (WITH_XL) xl = slow_engine_kernel<S, true>;
    return EngSlowEntry{S::D, S::H, S::HKV, S::HDIM, S::F, S::SQ, S::SF, S::SO, xl, slow_engine_kernel<S, false>};
}
template <typename S>
static EngFastEntry eng_fast_entry() {
    eng_fast_fn_t res = nullptr;
    if constexpr (S::RESF > 0) res = fast_engine_kernel<S, 10, true>;
    return EngFastEntry{S::D, S::H, S::HKV, S::HDIM, S::F, S::V, S::SQ, S::SF, S::SO, fast_engine_kernel<S, 10, false>, eng_qkv0_table_kernel<S>,
                        res, S::RESF, S::RESL};
}
static const EngSlowEntry* eng_slow_shapes(int* n) {
    static const EngSlowEntry tab[] = {eng_slow_entry<EngSlowS1, true>(), eng_slow_entry<EngSlowShape<1024, 16, 8, 128, 4096>, true>(),
                                       eng_slow_entry<EngSlowShape<1024, 16, 4, 128, 3072>, false>()};
    *n = (int)(sizeof tab / sizeof tab[0]);
    return tab;
}
static const EngFastEntry* eng_fast_shapes(int* n) {
    // (four fast kv heads of 64 would leave a workgroup 6 rows of Wqkv: not a whole number of 4-granule groups - such a model
    // keeps its codebook loop on launches)
    static const EngFastEntry tab[] = {eng_fast_entry<EngFastS1>(), eng_fast_entry<EngFastShape<1024, 16, 8, 64, 4096, 1024>>()};
    *n = (int)(sizeof tab / sizeof tab[0]);
    return tab;
}

// false: `why` says what kept the engine off (allocations made so far are released by the caller)
static bool eng_setup_try(ft_ctx* ctx, std::string& why) {
    const ft_ar_config& c = ctx->c;
    auto hip_ok = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        why = std::string(what) + ": " + hipGetErrorString(e);
        (void)hipGetLastError();     // (not sticky for the launch path)
        return false;
    };
    if (getenv("FT_NO_ENGINE")) { why = "FT_NO_ENGINE is set"; return false; }
    if (c.dtype != FT_BF16) { why = "precision is not bf16"; return false; }
    hipDeviceProp_t prop;
    if (!hip_ok(hipGetDeviceProperties(&prop, ctx->device), "hipGetDeviceProperties")) return false;
    const int nb = prop.multiProcessorCount;
    const int HD = c.n_head * c.head_dim;
    const int qkvN = (c.n_head + 2 * c.n_local_heads) * c.head_dim;
    auto per = [&](int units) { return (units + nb - 1) / nb; };
    // (the kernels carry the widths as compile-time constants: one instantiation per shape class)
    const EngSlowEntry* se = nullptr;
    {
        int n = 0;
        const EngSlowEntry* tab = eng_slow_shapes(&n);
        for (int i = 0; i < n && !se; ++i)
            if (c.dim == tab[i].D && c.n_head == tab[i].H && c.n_local_heads == tab[i].HKV && c.head_dim == tab[i].HDIM && c.intermediate_size == tab[i].F)
                se = &tab[i];
    }
    const bool shape_ok = se && c.fast_dim == c.dim && c.n_layer >= 1 && c.n_layer < ENG_EPOCH_STEP &&
                          per(qkvN) <= se->SQ * ENG_CW && per(c.dim) <= se->SO * ENG_CW && per(c.intermediate_size) <= se->SF * ENG_CW &&
                          qkvN % (4 * nb) == 0 && c.dim % (4 * nb) == 0 && c.intermediate_size % (4 * nb) == 0 && per(qkvN) <= ENG_LINE &&
                          per(c.intermediate_size) <= ENG_LINE && c.n_local_heads * ctx->nsplit_max <= nb && c.head_dim % (4 * ctx->nsplit_max) == 0 && nb == ENG_NB;
    if (!shape_ok) {
        char buf[320];
        snprintf(buf, sizeof buf, "widths outside the engine's instantiations (dim %d, heads %d / %d x %d, ffn %d, fast_dim %d on %d CUs; "
                 "built for dim 1024, 16 heads x 128 with 8 kv heads and ffn 3072 or 4096, or 4 kv heads and ffn 3072, on 256 CUs)", c.dim, c.n_head,
                 c.n_local_heads, c.head_dim, c.intermediate_size, c.fast_dim, nb);
        why = buf;
        return false;
    }
    {
        std::lock_guard<std::mutex> lk(g_eng_mu);
        auto it = g_eng_owner.find(ctx->device);
        if (it != g_eng_owner.end() && it->second != ctx) {
            why = "another context of this process already runs the frame engine on this device (its workgroups need every CU)";
            return false;
        }
        g_eng_owner[ctx->device] = ctx;
        ctx->eng_owner = true;
    }
    ctx->eng_nb = nb;
    std::vector<EngLayer> h(c.n_layer);
    for (int i = 0; i < c.n_layer; ++i) {
        const FtLayer& l = ctx->layers[i];
        h[i] = EngLayer{(const bf16_t*)l.wqkv, (const bf16_t*)l.bqkv, (const bf16_t*)l.attn_norm, (const bf16_t*)l.qn,
                        (const bf16_t*)l.kn, (const bf16_t*)l.wo, (const bf16_t*)l.bo, (const bf16_t*)l.ffn_norm,
                        (const bf16_t*)l.w13, (const bf16_t*)l.w2, (bf16_t*)l.kc, (bf16_t*)l.vc};
    }
    if (!hip_ok(hipMalloc((void**)&ctx->eng_layers, h.size() * sizeof(EngLayer)), "hipMalloc(engine layer table)")) return false;
    if (!hip_ok(hipMemcpy(ctx->eng_layers, h.data(), h.size() * sizeof(EngLayer), hipMemcpyHostToDevice), "hipMemcpy(engine layer table)")) return false;
    auto zalloc = [&](void** q, size_t bytes, const char* what) {
        return hip_ok(hipMalloc(q, bytes), what) && hip_ok(hipMemset(*q, 0, bytes), what);
    };
    const size_t L = c.n_layer;
    const size_t VB = (size_t)nb * ENG_LINE * 4;   // bytes reserved per hand-off vector (one 128-byte line per workgroup)
    // one pool [gx | gxb | gg | gy | gqkv], followed by the eight per-XCD replicas of it (XCD relay)
    const size_t pool_words = ((L + 1) * VB + 3 * L * VB + L * HD * 4) / 4;
    ctx->eng_relay = getenv("FT_NO_RELAY") == nullptr;
    ctx->eng_pool_bytes = pool_words * 4 * (ctx->eng_relay ? 9 : 1);
    if (!zalloc((void**)&ctx->eng_gx, ctx->eng_pool_bytes, "hipMalloc(engine hand-off pool)")) return false;
    ctx->eng_pool_words = pool_words;
    ctx->eng_gxb = ctx->eng_gx + (L + 1) * (VB / 4);
    ctx->eng_gg = ctx->eng_gxb + L * (VB / 4);
    ctx->eng_gy = ctx->eng_gg + L * (VB / 4);
    ctx->eng_gqkv = ctx->eng_gy + L * HD;
    ctx->eng_gpart_bytes = L * c.n_head * ctx->nsplit_max * (size_t)(c.head_dim + 2) * 8;
    if (!zalloc((void**)&ctx->eng_gpart, ctx->eng_gpart_bytes, "hipMalloc(engine split partials)")) return false;
    if (!zalloc((void**)&ctx->eng_ctl, ENG_CTL_WORDS * 4, "hipMalloc(engine control words)")) return false;
    const int G = c.n_head / c.n_local_heads, hd = c.head_dim, NSLOT = 4 * (64 / (hd >> 3));
    size_t fl = (size_t)c.dim * 2 + HD + c.intermediate_size + (size_t)(G + 2) * hd + (size_t)G * hd + 2 * hd +
                (size_t)NSLOT * G * 2 + (size_t)NSLOT * G * hd + 64 * 6 + ENG_MAX_OUT + 8;
    ctx->eng_lds_slow = std::max(fl * sizeof(float), (size_t)82 * 1024);   // > half the CU's LDS: one workgroup per CU
    const size_t lds_cap = prop.maxSharedMemoryPerMultiProcessor;
    if (ctx->eng_lds_slow > lds_cap) { why = "the slow stack's LDS need exceeds the CU's"; return false; }
    ctx->eng_xl = ctx->xl_shape && nb == 256 && ctx->nsplit_max == 32 && c.n_local_heads * 32 == nb;
    ctx->eng_xl = ctx->eng_xl && se->xl != nullptr;
    ctx->eng_slow_fn = (const void*)(ctx->eng_xl ? se->xl : se->plain);
    const void* slow_fn = ctx->eng_slow_fn;
    if (!hip_ok(hipFuncSetAttribute(slow_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->eng_lds_slow),
                "hipFuncSetAttribute(slow_engine_kernel)")) return false;
    // every workgroup must be resident at once, one per CU: does one fit a CU at all (registers, LDS, waves)?
    if (!eng_fits_cu(slow_fn, ctx->eng_lds_slow, lds_cap, "slow-stack", why)) return false;
    ctx->eng_on = true;
    why = ctx->eng_xl ? "slow stack on the frame engine (one kv head per XCD)" : "slow stack on the frame engine";

    // ---- fast codebook loop
    const int HDf = c.fast_n_head * c.fast_head_dim;
    const int fqkvN = (c.fast_n_head + 2 * c.fast_n_local_heads) * c.fast_head_dim;
    const EngFastEntry* fe = nullptr;
    {
        int n = 0;
        const EngFastEntry* tab = eng_fast_shapes(&n);
        for (int i = 0; i < n && !fe; ++i)
            if (c.fast_dim == tab[i].D && c.fast_n_head == tab[i].H && c.fast_n_local_heads == tab[i].HKV && c.fast_head_dim == tab[i].HDIM &&
                c.fast_intermediate_size == tab[i].F && ctx->fastV == tab[i].V)
                fe = &tab[i];
    }
    const bool fast_ok = !getenv("FT_NO_FAST_ENGINE") && fe && HDf == c.fast_dim && c.n_fast_layer >= 1 &&
                         c.num_codebooks >= 2 && c.num_codebooks <= 10 && fqkvN % (4 * nb) == 0 && ctx->fastV % (4 * nb) == 0 &&
                         per(fqkvN) <= fe->SQ * ENG_CW && per(c.fast_dim) <= fe->SO * ENG_CW && per(c.fast_intermediate_size) <= fe->SF * ENG_CW &&
                         per(ctx->fastV) <= fe->SO * ENG_CW && per(fqkvN) <= ENG_LINE && per(c.fast_intermediate_size) <= ENG_LINE && ctx->fastV <= 1024 &&
                         c.codebook_size <= 65536;
    if (!fast_ok) { why += "; fast loop on launches (FT_NO_FAST_ENGINE, or fast widths outside the instantiations: 1024 / 16 + 8 heads x 64 / ffn 3072 or 4096 / 1024 codes used, <= 10 codebooks)"; return true; }
    // the resident form needs every layer in its set; FT_NO_RESIDENT selects the all-streaming form (A/B runs, the equality test)
    const bool fast_res = fe->resident != nullptr && c.n_fast_layer <= fe->resl && getenv("FT_NO_RESIDENT") == nullptr;
    ctx->eng_fast_fn = (const void*)(fast_res ? fe->resident : fe->loop);
    // from here on a failure keeps the slow engine and leaves the fast loop on launches
    auto fast_off = [&](const std::string& w2) { why += "; fast loop on launches (" + w2 + ")"; return true; };
    std::vector<EngLayer> hf(c.n_fast_layer);
    for (int i = 0; i < c.n_fast_layer; ++i) {
        const FtLayer& l = ctx->flayers[i];
        hf[i] = EngLayer{(const bf16_t*)l.wqkv, (const bf16_t*)l.bqkv, (const bf16_t*)l.attn_norm, (const bf16_t*)l.qn,
                         (const bf16_t*)l.kn, (const bf16_t*)l.wo, (const bf16_t*)l.bo, (const bf16_t*)l.ffn_norm,
                         (const bf16_t*)l.w13, (const bf16_t*)l.w2, nullptr, nullptr};
    }
    std::string w2;
    auto hip_ok2 = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        w2 = std::string(what) + ": " + hipGetErrorString(e);
        (void)hipGetLastError();
        return false;
    };
    if (!hip_ok2(hipMalloc((void**)&ctx->eng_flayers, hf.size() * sizeof(EngLayer)), "hipMalloc(fast layer table)")) return fast_off(w2);
    if (!hip_ok2(hipMemcpy(ctx->eng_flayers, hf.data(), hf.size() * sizeof(EngLayer), hipMemcpyHostToDevice), "hipMemcpy(fast layer table)")) return fast_off(w2);
    const size_t nLf = c.n_fast_layer;
    // [2 parities]: gx (nLf + 1), gqkv, gxb, gg (nLf each), glog (1); then one line per codebook for the drawn codes
    ctx->eng_fast_words = (2 * ((nLf + 1) + 3 * nLf + 1)) * (VB / 4) + (size_t)c.num_codebooks * ENG_LINE;
    ctx->eng_fast_bytes = ctx->eng_fast_words * 4 * (ctx->eng_relay ? 9 : 1);
    if (!hip_ok2(hipMalloc((void**)&ctx->eng_fast_g, ctx->eng_fast_bytes), "hipMalloc(fast hand-off pool)") ||
        !hip_ok2(hipMemset(ctx->eng_fast_g, 0, ctx->eng_fast_bytes), "hipMemset(fast hand-off pool)")) return fast_off(w2);
    const int kvw = c.fast_n_local_heads * c.fast_head_dim;
    // codebook positions 0 and 1 as two rows of one pass when the second row's buffers fit the CU's LDS
    ctx->eng_pair = getenv("FT_NO_PAIR") == nullptr &&
                    eng_fast_lds_bytes(c.fast_dim, fqkvN, HDf, c.fast_intermediate_size, ctx->fastV, (int)nLf, c.num_codebooks, kvw, true) <= lds_cap;
    ctx->eng_lds_fast = eng_fast_lds_bytes(c.fast_dim, fqkvN, HDf, c.fast_intermediate_size, ctx->fastV, (int)nLf, c.num_codebooks, kvw, ctx->eng_pair);
    if (ctx->eng_lds_fast > lds_cap) return fast_off("the codebook loop's LDS need exceeds the CU's");
    ctx->eng_lds_fast = std::max(ctx->eng_lds_fast, (size_t)82 * 1024);
    if (!hip_ok2(hipFuncSetAttribute(ctx->eng_fast_fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)ctx->eng_lds_fast), "hipFuncSetAttribute(fast_engine_kernel)")) return fast_off(w2);
    if (!eng_fits_cu(ctx->eng_fast_fn, ctx->eng_lds_fast, lds_cap, "codebook-loop", w2)) return fast_off(w2);
    // layer 0's q k v of every codebook-embedding row a draw can select (codes < fastV): 4 MB at the s1-mini widths
    if (getenv("FT_NO_QKV0") == nullptr && c.num_codebooks > 2) {
        const size_t tb = (size_t)ctx->fastV * fqkvN * sizeof(bf16_t);
        if (!hip_ok2(hipMalloc((void**)&ctx->eng_qkv0_tab, tb), "hipMalloc(layer-0 q k v table)")) return fast_off(w2);
        const FtLayer& l0 = ctx->flayers[0];
        const size_t lds = ((size_t)c.fast_dim + ENG_MAX_OUT) * sizeof(float);
        fe->qkv0<<<dim3(fqkvN / (fe->SQ * ENG_CW), 16), ENG_CW * 64, lds, ctx->stream>>>(
            (const bf16_t*)l0.wqkv, (const bf16_t*)l0.bqkv, (const bf16_t*)l0.attn_norm, (const bf16_t*)ctx->fast_emb,
            (bf16_t*)ctx->eng_qkv0_tab, c.fast_dim, fqkvN, ctx->fastV, c.norm_eps);
        if (!hip_ok2(hipGetLastError(), "eng_qkv0_table_kernel") || !hip_ok2(hipStreamSynchronize(ctx->stream), "eng_qkv0_table_kernel")) {
            hipFree(ctx->eng_qkv0_tab); ctx->eng_qkv0_tab = nullptr;
            return fast_off(w2);
        }
    }
    ctx->eng_fast_on = true;
    why = ctx->eng_xl ? "slow stack (one kv head per XCD) and codebook loop on the frame engine" : "slow stack and codebook loop on the frame engine";
    {
        char buf[160];
        if (fast_res)
            snprintf(buf, sizeof buf, "; codebook loop: %d of %d W13 pairs per CU of %d layers resident in the gathering waves' registers",
                     fe->resf * ENG_GW, per(c.fast_intermediate_size), c.n_fast_layer);
        else
            snprintf(buf, sizeof buf, "; codebook loop: all weights streamed (%s)", fe->resident == nullptr ? "no resident set fits this shape class" :
                     c.n_fast_layer > fe->resl ? "more layers than the resident set holds" : "FT_NO_RESIDENT is set");
        why += buf;
    }
    return true;
}

static ft_status eng_setup(ft_ctx* ctx) {
    ctx->eng_on = ctx->eng_fast_on = false;
    std::string why;
    if (!eng_setup_try(ctx, why)) {
        eng_release(ctx);
        ctx->eng_why = "launch path: " + why;
    } else {
        char buf[64];
        snprintf(buf, sizeof buf, " (%d workgroups)", ctx->eng_nb);
        ctx->eng_why = why + buf;
    }
    if (getenv("FT_LOG")) fprintf(stderr, "fish_tts_amd: batch-1 decode frames: %s\n", ctx->eng_why.c_str());
    return FT_OK;
}

extern "C" ft_status ft_finalize_weights(ft_ctx* ctx) {
    if (!ctx) return FT_ERR_ARG;
    if (ctx->finalized) return FT_OK;
    FT_HIP(ctx, hipSetDevice(ctx->device));
    for (auto& kv : ctx->expected)
        if (!kv.second.p) return ft_fail(ctx, FT_ERR_MISSING_WEIGHT, "missing weight: " + kv.first);
    if (ctx->has_ar) FT_TRY(ar_finalize(ctx));
    if (ctx->has_codec) FT_TRY(codec_finalize(ctx));
    ctx->finalized = true;
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ launches
struct Launch {
    ft_ctx* ctx;
    hipStream_t s;
    int m0, M;       // batch rows [m0, m0+M)
    int pos_off;     // added to the device position (token-by-token prefill)
    hipError_t err = hipSuccess;
    bool gemv_only = false;  // measurement: enqueue only the weight-streaming GEMV launches of the frame
    bool tail_only = false;  // the frame tail follows a prompt pass: the rows' residual stream is in ctx->x (f32 rows)
    void chk() { hipError_t e = hipGetLastError(); if (e != hipSuccess && err == hipSuccess) err = e; }
};

// The model's type as template arguments: by_dtype(ctx, [&](auto t) { using T = decltype(t); f<typename T::WT, T::ROUND>(..); })
template <typename W, int R> struct DType { typedef W WT; static constexpr int ROUND = R; };
template <typename F>
static auto by_dtype(const ft_ctx* ctx, F&& f) {
    if (ctx->c.dtype == FT_BF16) return f(DType<bf16_t, RND_BF16>{});
    if (ctx->c.dtype == FT_F16) return f(DType<f16_t, RND_F16>{});
    return f(DType<float, RND_NONE>{});
}

// ---- launch trace of the AR frame (test hook, fishtts_hip_test.h).  A traced call appends one record per launch, in launch
// order; the launches of the armed range also copy every buffer they wrote to the host, WHOLE (every row of the allocation:
// the rows outside [m0, m0 + M) are there for the reader to compare with the record before), at that point of the stream.
// The copies read only: a traced call computes what an untraced one does.  Buffer ids (AR_TB_*): fishtts_hip_test.h.
enum { TB_X = 0, TB_QKV, TB_Y, TB_G, TB_LOGITS, TB_HID, TB_FEMB, TB_XF, TB_QKVF, TB_GF, TB_FLOG, TB_PART_O, TB_PART_ML,
       TB_PF_X = 13, TB_PF_QKV, TB_PF_Y,                         // the prompt pass's workspace: f32 rows [max_seq_len][width] ...
       TB_XO_X = 20, TB_XO_XF, TB_XO_FEMB, TB_XO_Y, TB_XO_G,
       TB_PF_XN = 25, TB_PF_YBF, TB_PF_QBF, TB_PF_G,             // ... and 16-bit rows [max_seq_len][width] (row-major, not octet-major)
       TB_TOKN = 30, TB_TOK, TB_POS, TB_NF, TB_DONE, TB_SEQ, TB_CUT, TB_CHUNK_CNT, TB_PART_IDX,
       TB_PROMPT = 39, TB_PF_SEQS, TB_PF_ROWS };                 // d_prompt [1][R max_seq_len], pf_seqs [max_batch][4], pf_rows [max_seq_len][2]
static const void* tr_buf(const ft_ctx* ctx, int id, int* esz, int* rows, int* cols) {
    const ft_ar_config& c = ctx->c;
    const int MB = c.max_batch, R = c.num_codebooks + 1, ldm = ctx->xo_ldm;
    const int qkvN = (c.n_head + 2 * c.n_local_heads) * c.head_dim, fqkvN = (c.fast_n_head + 2 * c.fast_n_local_heads) * c.fast_head_dim;
    const int HD = c.n_head * c.head_dim, HDf = c.fast_n_head * c.fast_head_dim, nchunk = (c.vocab_size + 1023) / 1024;
    *esz = 4;
    auto f = [&](const void* p, int r, int k) { *rows = r; *cols = k; return p; };
    auto o = [&](const void* p, int width) { *esz = 2; *rows = width / 8; *cols = ldm * 8; return p; };   // [width / 8][ldm][8]
    switch (id) {
        case TB_X: return f(ctx->x, MB, c.dim);
        case TB_QKV: return f(ctx->qkv, MB, qkvN);
        case TB_Y: return f(ctx->y, MB, ctx->y_ld);
        case TB_G: return f(ctx->g, MB, c.intermediate_size);
        case TB_LOGITS: return f(ctx->logits, MB, c.vocab_size);
        case TB_HID: return f(ctx->hid, MB, c.fast_dim);
        case TB_FEMB: return f(ctx->femb, MB, c.fast_dim);
        case TB_XF: return f(ctx->xf, MB, c.fast_dim);
        case TB_QKVF: return f(ctx->qkvf, 2 * ((MB + 15) / 16 * 16), fqkvN);
        case TB_GF: return f(ctx->gf, MB, c.fast_intermediate_size);
        case TB_FLOG: return f(ctx->flog, MB, ctx->fastV);
        case TB_PART_O: return f(ctx->part_o, 1, MB * c.n_head * ctx->nsplit_max * c.head_dim);
        case TB_PART_ML: return f(ctx->part_ml, 1, MB * c.n_head * ctx->nsplit_max * 2);
        case TB_XO_X: return o(ctx->xo_x, c.dim);
        case TB_XO_XF: return o(ctx->xo_xf, c.fast_dim);
        case TB_XO_FEMB: return o(ctx->xo_femb, c.fast_dim);
        case TB_XO_Y: return o(ctx->xo_y, std::max(HD, HDf));
        case TB_XO_G: return o(ctx->xo_g, std::max(c.intermediate_size, c.fast_intermediate_size));
        case TB_TOKN: return f(ctx->d_tokn, MB, R);
        case TB_TOK: return f(ctx->d_tok, MB, R);
        case TB_POS: return f(ctx->d_pos, 1, MB);
        case TB_NF: return f(ctx->d_nf, 1, MB);
        case TB_DONE: return f(ctx->d_done, 1, MB);
        case TB_SEQ: return f(ctx->d_seq, MB, R * ctx->cap);
        case TB_CUT: return f(ctx->samp_cut, MB, (int)(sizeof(SampCut) / 4));
        case TB_CHUNK_CNT: return f(ctx->samp_chunk_cnt, 1, MB * nchunk);
        case TB_PART_IDX: return f(ctx->samp_part_idx, 1, MB * nchunk);
        case TB_PF_X: return f(ctx->pf_x, c.max_seq_len, c.dim);
        case TB_PF_QKV: return f(ctx->pf_qkv, c.max_seq_len, qkvN);
        case TB_PF_Y: return f(ctx->pf_y, c.max_seq_len, HD);
        case TB_PF_XN: *esz = 2; return f(ctx->pf_xn, c.max_seq_len, c.dim);
        case TB_PF_YBF: *esz = 2; return f(ctx->pf_ybf, c.max_seq_len, HD);
        case TB_PF_QBF: *esz = 2; return f(ctx->pf_qbf, c.max_seq_len, HD);
        case TB_PF_G: *esz = 2; return f(ctx->pf_g, c.max_seq_len, c.intermediate_size);
        case TB_PROMPT: return f(ctx->d_prompt, 1, R * c.max_seq_len);
        case TB_PF_SEQS: return f(ctx->pf_seqs, MB, 4);
        case TB_PF_ROWS: return f(ctx->pf_rows, c.max_seq_len, 2);
    }
    return nullptr;
}
struct TrCls { int a = -1, b = -1, c = -1, d = -1; };
static void tr_rec(Launch& L, const std::string& name, int rows, int cols, TrCls cls, std::initializer_list<int> bufs) {
    ft_ctx* ctx = L.ctx;
    ArTrace& t = *ctx->trace;
    const int idx = (int)t.recs.size();
    t.recs.emplace_back();
    ArTraceRec& r = t.recs.back();
    // a prompt call: the pass in front of every name, the position in front of the position-by-position slow stack's
    r.name = t.pass_prefix + (name == "embed" || name.compare(0, 5, "slow.") == 0 ? t.pos_prefix : std::string()) + name;
    r.m0 = L.m0; r.rows = rows; r.cols = cols; r.pos_off = L.pos_off;
    r.cls[0] = cls.a; r.cls[1] = cls.b; r.cls[2] = cls.c; r.cls[3] = cls.d;
    r.held = idx >= t.first && idx < t.first + t.count;
    std::vector<int> ids(bufs);
    ids.insert(ids.end(), t.uploaded.begin(), t.uploaded.end());   // what the host uploaded for this pass rides with its first launch
    t.uploaded.clear();
    for (int id : ids) {
        ArTraceBuf b;
        const void* p = tr_buf(ctx, id, &b.esz, &b.rows, &b.cols);
        if (!p) continue;
        b.id = id;
        if (r.held) {
            b.data.resize((size_t)b.rows * b.cols * b.esz);
            if (hipMemcpyAsync(b.data.data(), p, b.data.size(), hipMemcpyDeviceToHost, L.s) != hipSuccess) t.failed = true;
        }
        r.bufs.push_back(std::move(b));
    }
    if (r.held && hipStreamSynchronize(L.s) != hipSuccess) t.failed = true;
}
static std::string tr_name(const char* fmt, ...) {
    char buf[64];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}
// The trace's name of a layer's launch, <stack>.<n>.<op> (slow.3.wo, fast.2.0.wqkv, fast.pair.1.attn; the codebook heads are
// fast.<cb>.head), or <op> alone (fproj, head).  Formatted only while a trace is active.
struct TrName {
    const char* stack; int n; const char* op;
    std::string str() const { return stack ? tr_name("%s.%d.%s", stack, n, op) : std::string(op); }
};
// A working buffer from the launch's first row on, with its trace id: f32 rows, or octet-major 16-bit elements (wide_kernels.h)
struct RowBuf { float* p; int id; };
struct XoBuf { bf16_t* p; int id; };
// d_tok, d_pos, d_nf, d_done and the frame store d_seq of every slot (which: 0 before the first launch, 1 after the call)
static void tr_state(ft_ctx* ctx, int which) {
    ArTrace& t = *ctx->trace;
    ArTraceState& s = t.st[which];
    const size_t MB = ctx->c.max_batch, R = ctx->c.num_codebooks + 1;
    s.tok.resize(MB * R); s.pos.resize(MB); s.nf.resize(MB); s.done.resize(MB); s.seq.resize(MB * R * ctx->cap);
    bool ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
    ok = ok && hipMemcpy(s.tok.data(), ctx->d_tok, s.tok.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(s.pos.data(), ctx->d_pos, MB * 4, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(s.nf.data(), ctx->d_nf, MB * 4, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(s.done.data(), ctx->d_done, MB * 4, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(s.seq.data(), ctx->d_seq, s.seq.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (which == 0) {   // and every buffer a launch can write, as the call found it: the record before a buffer's first write
        static const int ids[] = {TB_X, TB_QKV, TB_Y, TB_G, TB_LOGITS, TB_HID, TB_FEMB, TB_XF, TB_QKVF, TB_GF, TB_FLOG, TB_PART_O, TB_PART_ML,
                                  TB_XO_X, TB_XO_XF, TB_XO_FEMB, TB_XO_Y, TB_XO_G, TB_TOKN, TB_TOK, TB_POS, TB_NF, TB_DONE, TB_SEQ, TB_CUT,
                                  TB_CHUNK_CNT, TB_PART_IDX};
        static const int pf_ids[] = {TB_PF_X, TB_PF_QKV, TB_PF_Y, TB_PF_XN, TB_PF_YBF, TB_PF_QBF, TB_PF_G, TB_PROMPT, TB_PF_SEQS, TB_PF_ROWS};
        std::vector<int> all(std::begin(ids), std::end(ids));
        if (t.kind >= 3) all.insert(all.end(), std::begin(pf_ids), std::end(pf_ids));     // a prompt call: its workspace too
        t.begin.clear();
        for (int id : all) {
            ArTraceBuf b;
            const void* p = tr_buf(ctx, id, &b.esz, &b.rows, &b.cols);
            if (!p) continue;
            b.id = id;
            b.data.resize((size_t)b.rows * b.cols * b.esz);
            ok = ok && hipMemcpy(b.data.data(), p, b.data.size(), hipMemcpyDeviceToHost) == hipSuccess;
            t.begin.push_back(std::move(b));
        }
    }
    if (!ok) t.failed = true;
}
// A traced call: armed -> active for this call only (kind: 1 a decode frame, 2 first frames, 3 ft_ar_prefill_at, 4
// ft_ar_prefill_slow, 5 ft_ar_prefill_slow_many).  A call made inside a traced one (the single passes ft_ar_prefill_slow_many falls
// back to) finds the trace active and leaves it alone: `own` is false there, and so is it in an untraced call.
struct ArTraceScope {
    ft_ctx* ctx;
    bool own = false;
    ArTraceScope(ft_ctx* c, bool eligible, int kind, int m0, int M) : ctx(c) {
        ArTrace& t = ctx->tstore;
        if (ctx->trace || !t.armed) return;
        t.armed = false;
        if (!eligible) return;
        t.recs.clear(); t.uploaded.clear(); t.pass_prefix.clear(); t.pos_prefix.clear();
        t.failed = false; t.kind = kind; t.m0 = m0; t.M = M;
        ctx->trace = &t;
        own = true;
    }
    ~ArTraceScope() { if (own) ctx->trace = nullptr; }
};
// the host uploaded these buffers for the pass about to start: the pass's first launch record carries them
static void tr_uploaded(ft_ctx* ctx, std::initializer_list<int> ids) { if (ctx->trace) ctx->trace->uploaded.assign(ids); }
static void tr_pos(ft_ctx* ctx, int t) { if (ctx->trace) ctx->trace->pos_prefix = tr_name("t%d.", t); }

struct PfX {   // fused RMSNorm hooks of the skinny kernel (gemm_kernels.h TapGemmP)
    const void* gain = nullptr;   // normalise the X rows with this gain ...
    const float* ss_in = nullptr; // ... and the producer's partial sums of squares (nblk per row)
    int nblk = 0;
    float* ss_out = nullptr;      // leave this GEMM's own partials for the next consumer
};
// Returns which kernel class ran (PF_ID_*, include/fishtts_hip_test.h: ft_test_pf_linear reports it; prefill_gemm ignores it).
enum { PF_ID_NONE = -1, PF_ID_SKINNY1 = 0, PF_ID_SKINNY2 = 1, PF_ID_SKINNY4 = 2, PF_ID_LIN128 = 3, PF_ID_LIN64 = 4, PF_ID_TAP64_128 = 5,
       PF_ID_TAP64_64 = 6, PF_ID_TAP_128 = 7, PF_ID_TAP_64 = 8 };
static int pf_gemm(Launch& L, const bf16_t* X, long ldx, int S, const void* W, const float* bias, int N, int K,
                   int act, const float* resid, float* out_f32, bf16_t* out_bf, long ldo, int round_out,
                   const PfX& fx = PfX());
// A lock-step batch of >= wide_min rows (bf16 or fp16): every Linear is ONE M-row MFMA launch (weights read once for the whole
// batch) with the RMSNorm / SwiGLU / residual add folded in (wide_kernels.h): five launches per layer.
static bool wide_batch(const Launch& L) {
    return L.ctx->wide_ok && L.M >= L.ctx->wide_min && L.M <= 64 && !L.gemv_only && !L.ctx->prof;
}

// Codebook positions 0 and 1 of a wide batch in ONE pass of 2 M rows (both inputs are known once the semantic token is drawn:
// the slow stack's hidden state and the drawn code's embedding, inference.py:116-131): rows xo_pair + m hold position 1.
static bool wide_pair(const Launch& L) {
    const ft_ctx* ctx = L.ctx;
    return wide_batch(L) && !ctx->no_pair && ctx->c.num_codebooks >= 2 && ctx->c.n_fast_layer > 0 && ctx->xo_pair + L.M <= 64;
}

// One Linear of a lock-step batch.  Tile choices per shape class measured with tools/mb_wide.hip (profiles/r04_mb_wide.txt):
// two 16-row weight tiles per workgroup where the fused norm's arithmetic would otherwise be paid per 16 rows of a long
// matrix (W13 always, Wqkv from 17 batch rows), both 16-row batch tiles in one workgroup only where the weights
// dominate (W13, the vocabulary head); everything else splits the batch rows over workgroups.
// WT: the model's 16-bit element type; the octet-major buffers of the context are raw 16-bit storage (declared bf16_t)
// Returns which instantiation class ran (WIDE_ID_*, include/fishtts_hip_test.h: ft_test_wide_linear reports it).
enum { WIDE_ID_S11 = 0, WIDE_ID_S12 = 1, WIDE_ID_S22 = 2, WIDE_ID_G12 = 3, WIDE_ID_G22 = 4, WIDE_ID_R11 = 5, WIDE_ID_HEAD = 6 };
template <typename WT>
static int wide_gemm(Launch& L, const bf16_t* X, const void* W, const float* bias, int N, int K, const void* gain, int epi,
                      float* out_f32, long ldo, bf16_t* out_xo, const bf16_t* resid_xo, int rows = 0, bool vocab_head = false) {
    const int M = rows > 0 ? rows : L.M;
    WidePT<WT> p{};
    p.X = (const WT*)X; p.ldm = L.ctx->xo_ldm; p.W = (const WT*)W; p.ldw = K; p.gain = (const WT*)gain; p.eps = L.ctx->c.norm_eps;
    p.bias = bias; p.M = M; p.N = N; p.K = K; p.out_f32 = out_f32; p.ldo = ldo; p.out_xo = (WT*)out_xo; p.ldm_o = L.ctx->xo_ldm;
    p.resid_xo = (const WT*)resid_xo;
    bool ok;
    int id;
    if (epi == WEPI_RESID) { id = WIDE_ID_R11; ok = wide_gemm_launch<1, 1, false, WEPI_RESID>(p, L.s); }
    else if (epi == WEPI_SWIGLU) {
        id = M > 16 ? WIDE_ID_G22 : WIDE_ID_G12;
        ok = M > 16 ? wide_gemm_launch<2, 2, true, WEPI_SWIGLU>(p, L.s) : wide_gemm_launch<1, 2, true, WEPI_SWIGLU>(p, L.s);
    }
    else if (vocab_head && M <= 32 && K == 1024 && N % 16 == 0 && N >= 4096 && !L.ctx->no_head_stream) {
        // the vocabulary head: activations normalised once per workgroup, weights streamed per wave (wide_head_kernel)
        static DevOnce once;
        once.run([] { hipFuncSetAttribute((const void*)wide_head_kernel<1024, WT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wide_head_lds<1024>()); });
        wide_head_kernel<1024, WT><<<256, 512, wide_head_lds<1024>(), L.s>>>(p);
        id = WIDE_ID_HEAD;
        ok = true;
    }
    else if (N >= 32768) {
        id = M > 16 ? WIDE_ID_S22 : WIDE_ID_S12;
        ok = M > 16 ? wide_gemm_launch<2, 2, true, WEPI_STORE>(p, L.s) : wide_gemm_launch<1, 2, true, WEPI_STORE>(p, L.s);
    }
    else if (N >= 4096 && M > 16) { id = WIDE_ID_S12; ok = wide_gemm_launch<1, 2, true, WEPI_STORE>(p, L.s); }
    else { id = WIDE_ID_S11; ok = wide_gemm_launch<1, 1, true, WEPI_STORE>(p, L.s); }
    if (!ok && L.err == hipSuccess) L.err = hipErrorInvalidValue;
    L.chk();
    return id;
}
// A Linear of the frame on that launch, with its trace record: the output is f32 rows (WEPI_STORE) or octet-major
template <typename WT>
static void wide_linear(Launch& L, const TrName& nm, const bf16_t* X, const void* W, const float* bias, const void* gain, int N, int K,
                        int epi, RowBuf out_f32, long ldo, XoBuf out_xo, const bf16_t* resid_xo, int rows = 0, bool vocab_head = false) {
    const int id = wide_gemm<WT>(L, X, W, bias, N, K, gain, epi, out_f32.p, ldo, out_xo.p, resid_xo, rows, vocab_head);
    if (L.ctx->trace) tr_rec(L, nm.str(), rows > 0 ? rows : L.M, epi == WEPI_SWIGLU ? N / 2 : N, TrCls{id}, {out_xo.p ? out_xo.id : out_f32.id});
}

// f32 rows -> octet-major 16-bit elements (the values are exact in the model's type): the residual stream a prompt pass left in ctx->x
template <typename WT>
static __global__ __launch_bounds__(256) void xo_from_rows_kernel(const float* x, int ldx, int D, bf16_t* xo, int ldm) {
    const int m = blockIdx.y;
    for (int d = blockIdx.x * 256 + threadIdx.x; d < D; d += gridDim.x * 256) xo[xo_index(m, d, ldm)] = h16_bits<WT>(x[(size_t)m * ldx + d]);
}

// 16-bit rows [row][D] -> octet-major operand rows (table build below; a copy of bits, either type)
static __global__ __launch_bounds__(256) void xo_from_h16_rows_kernel(const bf16_t* x, int D, bf16_t* xo, int ldm, int rows) {
    const int m = blockIdx.y;
    if (m >= rows) return;
    for (int d = blockIdx.x * 256 + threadIdx.x; d < D; d += gridDim.x * 256) xo[xo_index(m, d, ldm)] = x[(size_t)m * D + d];
}
template <typename WT>
static __global__ void f32_to_h16_kernel(const float* x, bf16_t* o, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) o[i] = h16_bits<WT>(x[i]);
}

// Wide batches: the table of layer 0's q k v for every code a codebook draw can select (codes < fastV), built at load with
// the very launch that would compute those rows in a frame (the rows of a lock-step GEMM do not depend on each other, so a
// table row carries the bits the launch would produce): 4 MB at the s1-mini widths, one launch less per codebook step.
template <typename WT>
static ft_status wide_qkv0_build_t(ft_ctx* ctx) {
    const ft_ar_config& c = ctx->c;
    if (!ctx->wide_ok || getenv("FT_NO_QKV0") || c.num_codebooks <= 2 || c.n_fast_layer < 1) return FT_OK;
    const int Df = c.fast_dim, qkvN = (c.fast_n_head + 2 * c.fast_n_local_heads) * c.fast_head_dim, V = ctx->fastV;
    const FtLayer& l0 = ctx->flayers[0];
    if (l0.bqkv) return FT_OK;
    constexpr int CH = 64;
    bf16_t* xo = nullptr; float* out = nullptr;
    if (hipMalloc((void**)&xo, (size_t)Df * CH * sizeof(bf16_t)) != hipSuccess || hipMalloc((void**)&out, (size_t)CH * qkvN * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&ctx->wide_qkv0_tab, (size_t)V * qkvN * sizeof(bf16_t)) != hipSuccess) {
        (void)hipGetLastError();
        if (xo) hipFree(xo);
        if (out) hipFree(out);
        if (ctx->wide_qkv0_tab) { hipFree(ctx->wide_qkv0_tab); ctx->wide_qkv0_tab = nullptr; }
        return FT_OK;      // the frames then keep their layer-0 launch
    }
    bool ok = true;
    for (int c0 = 0; c0 < V && ok; c0 += CH) {
        const int rows = std::min(CH, V - c0);
        xo_from_h16_rows_kernel<<<dim3((Df + 255) / 256, rows), 256, 0, ctx->stream>>>((const bf16_t*)ctx->fast_emb + (size_t)c0 * Df, Df, xo, CH, rows);
        WidePT<WT> p{};
        p.X = (const WT*)xo; p.ldm = CH; p.W = (const WT*)l0.wqkv; p.ldw = Df; p.gain = (const WT*)l0.attn_norm; p.eps = c.norm_eps;
        p.M = rows; p.N = qkvN; p.K = Df; p.out_f32 = out; p.ldo = qkvN;
        ok = wide_gemm_launch<1, 1, true, WEPI_STORE>(p, ctx->stream);
        f32_to_h16_kernel<WT><<<256, 256, 0, ctx->stream>>>(out, ctx->wide_qkv0_tab + (size_t)c0 * qkvN, (long)rows * qkvN);
    }
    ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess && hipGetLastError() == hipSuccess;
    hipFree(xo); hipFree(out);
    if (!ok) { hipFree(ctx->wide_qkv0_tab); ctx->wide_qkv0_tab = nullptr; (void)hipGetLastError(); }
    return FT_OK;
}
static ft_status wide_qkv0_build(ft_ctx* ctx) {
    if (ctx->c.dtype == FT_BF16) return wide_qkv0_build_t<bf16_t>(ctx);
    if (ctx->c.dtype == FT_F16) return wide_qkv0_build_t<f16_t>(ctx);
    return FT_OK;
}

static bool eng_slow_ok(const Launch& L) {
    const ft_ctx* ctx = L.ctx;
    return ctx->eng_on && !ctx->eng_suspended && L.M == 1 && !L.gemv_only && !ctx->prof && ctx->c.n_local_heads * ctx->nsplit <= ctx->eng_nb &&
           ctx->c.head_dim % (4 * ctx->nsplit) == 0;
}

static bool eng_fast_ok(const Launch& L) {
    const ft_ctx* ctx = L.ctx;
    return ctx->eng_fast_on && !ctx->eng_suspended && L.M == 1 && !L.gemv_only && !ctx->prof;
}

// The whole codebook loop of one frame (steps 0 .. num_codebooks-1 with their draws) as one launch; runs after the
// vocabulary head + semantic draw launches, which leave the hidden state, the first code's embedding and tokn[0..1].
static void enqueue_fast_engine(Launch& L) {
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const int m0 = L.m0, R = c.num_codebooks + 1, nb = ctx->eng_nb;
    const size_t nLf = c.n_fast_layer, VW = (size_t)nb * ENG_LINE;
    FastEngP p{};
    p.layers = ctx->eng_flayers; p.n_layer = c.n_fast_layer; p.ncb = c.num_codebooks;
    p.D = c.fast_dim; p.H = c.fast_n_head; p.Hkv = c.fast_n_local_heads; p.hd = c.fast_head_dim; p.F = c.fast_intermediate_size;
    p.qkvN = (c.fast_n_head + 2 * c.fast_n_local_heads) * c.fast_head_dim; p.V = ctx->fastV;
    p.eps = c.norm_eps; p.scale = (float)(1.0 / sqrt((double)c.fast_head_dim));
    p.rope = ctx->frope; p.fast_norm = (const bf16_t*)ctx->fast_norm; p.fast_out = (const bf16_t*)ctx->fast_out;
    p.fast_emb = (const bf16_t*)ctx->fast_emb;
    p.qkv0_tab = (const bf16_t*)ctx->eng_qkv0_tab;
    p.hid = ctx->hid + (size_t)m0 * c.fast_dim; p.femb = ctx->femb + (size_t)m0 * c.fast_dim;
    unsigned* g = ctx->eng_fast_g;
    p.gx = g; g += 2 * (nLf + 1) * VW;
    p.gqkv = g; g += 2 * nLf * VW;
    p.gxb = g; g += 2 * nLf * VW;
    p.gg = g; g += 2 * nLf * VW;
    p.glog = g; g += 2 * VW;
    p.gcode = g;
    p.ctl = ctx->eng_ctl;
    p.rep_delta0 = ctx->eng_relay ? (long)ctx->eng_fast_words : 0; p.rep_stride = ctx->eng_relay ? (long)ctx->eng_fast_words : 0;
    SampP s{};
    s.logits = nullptr; s.ldl = ctx->fastV; s.V = ctx->fastV;
    s.ctl = ctx->d_ctl + m0; s.tokn = ctx->d_tokn + (size_t)m0 * R; s.seq = ctx->d_seq + (size_t)m0 * R * ctx->cap;
    s.cap = ctx->cap; s.nf = ctx->d_nf + m0; s.cb = 1; s.ncb = c.num_codebooks; s.sem_begin = c.semantic_begin_id;
    s.im_end = c.im_end_id; s.cbsize = c.codebook_size; s.fast_emb = ctx->fast_emb;
    s.femb = ctx->femb + (size_t)m0 * c.fast_dim; s.Df = c.fast_dim; s.noise = ctx->noise;
    s.noise_row_len = ctx->noise_row_len; s.noise_rows = ctx->noise_rows; s.noise_off = 0; s.last = 0;
    s.tok = ctx->d_tok + (size_t)m0 * R; s.pos = ctx->d_pos + m0; s.done = ctx->d_done + m0;
    p.samp = s;
    p.noise_cb_stride = ctx->fastV; p.noise_off1 = c.vocab_size;
    p.pair = ctx->eng_pair ? 1 : 0;
    ((eng_fast_fn_t)ctx->eng_fast_fn)<<<nb, ENG_THREADS, ctx->eng_lds_fast, L.s>>>(p);
    L.chk();
}

static void enqueue_slow_engine(Launch& L, const int* toks, long tok_row_stride, long tok_m_stride, int col) {
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const int m0 = L.m0;
    SlowEngP p{};
    p.layers = ctx->eng_layers; p.n_layer = c.n_layer;
    p.D = c.dim; p.H = c.n_head; p.Hkv = c.n_local_heads; p.hd = c.head_dim; p.F = c.intermediate_size;
    p.qkvN = (c.n_head + 2 * c.n_local_heads) * c.head_dim;
    p.eps = c.norm_eps; p.scale = 1.0f / sqrtf((float)c.head_dim);
    p.emb = (const bf16_t*)ctx->emb; p.cb_emb = (const bf16_t*)ctx->cb_emb;
    p.toks = toks + (size_t)m0 * tok_m_stride + col; p.tok_row_stride = tok_row_stride;
    p.ncb = c.num_codebooks; p.cbsize = c.codebook_size; p.vocab = c.vocab_size; p.sem_begin = c.semantic_begin_id;
    p.sem_end = c.semantic_end_id; p.scale_cb = c.scale_codebook_embeddings; p.inv_div = (float)sqrt((double)(c.num_codebooks + 1));
    p.rope = ctx->rope; p.pos = ctx->d_pos + m0; p.pos_off = L.pos_off; p.n_slots = ctx->n_slots; p.nsplit = ctx->nsplit;
    p.cache_off = (size_t)m0 * ctx->cache_m_stride;
    p.gx = ctx->eng_gx; p.gqkv = ctx->eng_gqkv; p.gpart = ctx->eng_gpart; p.gy = ctx->eng_gy; p.gxb = ctx->eng_gxb; p.gg = ctx->eng_gg;
    p.ctl = ctx->eng_ctl; p.x_out = ctx->x + (size_t)m0 * c.dim; p.nt = 1;
    p.rep_delta0 = ctx->eng_relay ? (long)ctx->eng_pool_words : 0; p.rep_stride = ctx->eng_relay ? (long)ctx->eng_pool_words : 0;
    ((eng_slow_fn_t)ctx->eng_slow_fn)<<<ctx->eng_nb, ENG_THREADS, ctx->eng_lds_slow, L.s>>>(p);
    L.chk();
}


template <typename WT, int ROUND, int R>
static void gemv_nt(Launch& L, const GemvP& p, int nt) {
    const dim3 grid((p.N + 4 * R - 1) / (4 * R), L.M), block(256);
#define FT_NT(n) case n: gemv_kernel<WT, n, R, ROUND><<<grid, block, 0, L.s>>>(p); break;
    switch (nt) { FT_NT(1) FT_NT(2) FT_NT(3) FT_NT(4) FT_NT(6) FT_NT(8) FT_NT(12) default: L.err = hipErrorInvalidValue; }
#undef FT_NT
}

static int pick_nt(int K, int vec) {
    const int need = (K + 64 * vec - 1) / (64 * vec);
    const int opts[] = {1, 2, 3, 4, 6, 8, 12};
    for (int o : opts) if (o >= need) return o;
    return -1;
}

template <typename WT, int ROUND, int R, int MB>
static void gemv_mb_nt(Launch& L, const GemvP& p, int nt) {
    const dim3 grid((p.N + 4 * R - 1) / (4 * R), (L.M + MB - 1) / MB), block(256);
#define FT_NT(n) case n: gemv_mb_kernel<WT, n, R, MB, ROUND><<<grid, block, 0, L.s>>>(p, L.M); break;
    switch (nt) { FT_NT(1) FT_NT(2) FT_NT(4) FT_NT(6) default: L.err = hipErrorInvalidValue; }
#undef FT_NT
}

// Returns what it launched (the test hook ft_test_gemv reports it; the frames ignore it): MB rows per pass over the weights
// (0: gemv_kernel, one grid row per batch row), R weight rows per wave, NT 16-byte pieces of K per lane.
struct GemvId { int MB, R, NT; };
template <typename WT, int ROUND>
static GemvId gemv(Launch& L, GemvP p, int R) {
    const int nt = pick_nt(p.K, Vec<WT>::N);
    if (nt < 0) { L.err = hipErrorInvalidValue; return GemvId{-1, -1, -1}; }
    GemvId id{0, 0, nt};
    ft_ctx* ctx = L.ctx;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->prof && !ctx->prof_count_only) {
        hipEventCreate(&e0); hipEventCreate(&e1);
        hipEventRecord(e0, L.s);
    }
    if (p.epi == EPI_SWIGLU && R < 2) R = 2;
    // lock-step batches (bf16): several utterance rows per pass over the weights
    const bool mb_ok = sizeof(WT) == 2 && L.M >= 2 && (nt == 1 || nt == 2 || nt == 4 || nt == 6);
    if (mb_ok) {
        if constexpr (sizeof(WT) == 2) {
            const bool four = L.M >= 3 && nt <= 2 && R <= 2;  // register budget: 4 x NT x 8 activations
            if (R >= 4) { id.R = 4; if (nt <= 2) { id.MB = 2; gemv_mb_nt<WT, ROUND, 4, 2>(L, p, nt); } else gemv_nt<WT, ROUND, 4>(L, p, nt); }
            else if (R == 2) { id.R = 2; id.MB = four ? 4 : 2; if (four) gemv_mb_nt<WT, ROUND, 2, 4>(L, p, nt); else gemv_mb_nt<WT, ROUND, 2, 2>(L, p, nt); }
            else { id.R = 1; id.MB = four ? 4 : 2; if (four) gemv_mb_nt<WT, ROUND, 1, 4>(L, p, nt); else gemv_mb_nt<WT, ROUND, 1, 2>(L, p, nt); }
        }
    } else if (R == 1) { id.R = 1; gemv_nt<WT, ROUND, 1>(L, p, nt); }
    else if (R == 2) { id.R = 2; gemv_nt<WT, ROUND, 2>(L, p, nt); }
    else if (R >= 8 && nt <= 2 && p.epi != EPI_SWIGLU) { id.R = 8; gemv_nt<WT, ROUND, 8>(L, p, nt); }
    else { id.R = 4; gemv_nt<WT, ROUND, 4>(L, p, nt); }
    if (ctx->prof) {
        if (!ctx->prof_count_only) {
            hipEventRecord(e1, L.s);
            ctx->prof_ev.push_back(e0); ctx->prof_ev.push_back(e1);
        }
        ctx->prof_bytes += (int64_t)p.N * p.K * sizeof(WT);
        ctx->prof_launches += 1;
    }
    L.chk();
    return id;
}

static int rows_per_wave(int N, int M) {
    // enough waves to cover the chip (256 CUs x 4 SIMDs) a few times over; big matrices amortise
    const long waves1 = (long)N * M;
    // (the vocabulary head, 155 776 rows at M = 1: 8 rows per wave - 16 KB in flight - measured 0.5 % slower than 4)
    if (waves1 >= 65536) return 4;
    if (waves1 >= 2048) return 2;
    return 1;
}

// A Linear of the frame on the GEMV launches.  The frame's GemvP are filled here and nowhere else: a gain selects the RMSNorm
// prologue, a residual (rows of the output's stride) belongs to EPI_RESID, ldo is the stride of the output rows (N / 2
// columns under EPI_SWIGLU).  gemv_launch runs a filled one and owns its trace record.
static GemvP gemv_params(const ft_ctx* ctx, const void* W, const void* bias, const void* gain, const float* x, int ldx, float* out, int ldo,
                         const float* resid, int N, int K, int epi, int nt) {
    GemvP p{};
    p.W = W; p.bias = bias; p.x = x; p.ldx = ldx; p.gain = gain; p.eps = gain ? ctx->c.norm_eps : 0.f;
    p.out = out; p.ldo = ldo; p.resid = resid; p.ldr = resid ? ldo : 0; p.N = N; p.K = K;
    p.pro = gain ? PRO_RMSNORM : PRO_NONE; p.epi = epi; p.nt = nt;
    return p;
}
template <typename WT, int ROUND>
static void gemv_launch(Launch& L, const TrName& nm, int buf, const GemvP& p) {
    const GemvId id = gemv<WT, ROUND>(L, p, rows_per_wave(p.N, L.M));
    if (L.ctx->trace) tr_rec(L, nm.str(), L.M, p.epi == EPI_SWIGLU ? p.N / 2 : p.N, TrCls{id.MB, id.R, id.NT}, {buf});
}
template <typename WT, int ROUND>
static void gemv_linear(Launch& L, const TrName& nm, const void* W, const void* bias, const void* gain, const float* x, int ldx, RowBuf out,
                        int ldo, const float* resid, int N, int K, int epi, int nt) {
    gemv_launch<WT, ROUND>(L, nm, out.id, gemv_params(L.ctx, W, bias, gain, x, ldx, out.p, ldo, resid, N, K, epi, nt));
}

template <typename WT, int ROUND>
static void attn_decode(Launch& L, const AttnP& p) {
    ft_ctx* ctx = L.ctx;
    const int G = p.H / p.Hkv;
    const int nslot = 2048 / p.hd;
    const size_t lds = ((size_t)G * p.hd + 2 * p.hd + (size_t)nslot * G * 2 + (size_t)nslot * G * p.hd) * sizeof(float);
    const dim3 grid(p.Hkv, p.nsplit, L.M), block(256);
    switch (G) {
        case 1: attn_decode_kernel<WT, 1, ROUND><<<grid, block, lds, L.s>>>(p); break;
        case 2: attn_decode_kernel<WT, 2, ROUND><<<grid, block, lds, L.s>>>(p); break;
        case 4: attn_decode_kernel<WT, 4, ROUND><<<grid, block, lds, L.s>>>(p); break;
        case 8: {
            static DevOnce once;     // per device (the opt-in belongs to the current device's function object)
            once.run([&] { hipFuncSetAttribute((const void*)attn_decode_kernel<WT, 8, ROUND>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
            attn_decode_kernel<WT, 8, ROUND><<<grid, block, lds, L.s>>>(p);
            break;
        }
        default: L.err = hipErrorInvalidValue;
    }
    L.chk();
    (void)ctx;
}

template <typename WT, int ROUND, int R>
static void gemv_combine_nt(Launch& L, const GemvP& p, const AttnP& a, int nt) {
    const dim3 grid((p.N + 4 * R - 1) / (4 * R), L.M), block(256);
#define FT_NT(n) case n: gemv_attn_combine_kernel<WT, n, R, ROUND><<<grid, block, (size_t)a.H * a.hd * sizeof(float), L.s>>>(p, a); break;
    switch (nt) { FT_NT(1) FT_NT(2) FT_NT(3) FT_NT(4) FT_NT(6) FT_NT(8) FT_NT(12) default: L.err = hipErrorInvalidValue; }
#undef FT_NT
}

// The "decode attention, then Wo" part of a slow layer for 1..max_batch rows: attn_decode_kernel over ctx->nsplit KV splits, then the
// Wo product with the residual add - with more than one split the partials are merged inside it (gemv_attn_combine_kernel),
// with one it reads the attention's y.  enqueue_slow's attention step and the test hook ft_test_decode_attn both call it.
template <typename WT, int ROUND>
static void decode_attn_wo(Launch& L, const AttnP& a, const GemvP& o, int li = -1) {
    ft_ctx* ctx = L.ctx;
    if (!L.gemv_only) attn_decode<WT, ROUND>(L, a);
    if (ctx->trace) {
        if (ctx->nsplit > 1) tr_rec(L, tr_name("slow.%d.attn", li), L.M, a.H * a.hd, TrCls{ctx->nsplit}, {TB_PART_O, TB_PART_ML});
        else tr_rec(L, tr_name("slow.%d.attn", li), L.M, a.H * a.hd, TrCls{1}, {TB_Y});
    }
    if (ctx->nsplit > 1) {  // split-KV partials are merged inside the Wo kernel
        const int nt = pick_nt(o.K, Vec<WT>::N);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (ctx->prof && !ctx->prof_count_only) { hipEventCreate(&e0); hipEventCreate(&e1); hipEventRecord(e0, L.s); }
        if (rows_per_wave(o.N, L.M) >= 2) gemv_combine_nt<WT, ROUND, 2>(L, o, a, nt);
        else gemv_combine_nt<WT, ROUND, 1>(L, o, a, nt);
        if (ctx->trace) tr_rec(L, tr_name("slow.%d.wo", li), L.M, o.N, TrCls{-2, rows_per_wave(o.N, L.M) >= 2 ? 2 : 1, nt}, {TB_X});
        if (ctx->prof) {
            if (!ctx->prof_count_only) {
                hipEventRecord(e1, L.s);
                ctx->prof_ev.push_back(e0); ctx->prof_ev.push_back(e1);
            }
            ctx->prof_bytes += (int64_t)o.N * o.K * sizeof(WT);
            ctx->prof_launches += 1;
        }
        L.chk();
    } else {
        gemv_launch<WT, ROUND>(L, TrName{"slow", li, "wo"}, TB_X, o);
    }
}

// The slow-stack attention launch of a wide batch, on an AttnP filled but for the split fields.  >= 128 (row, kv head)
// blocks: each walks its row's whole context with the two-pass kernel; fewer rows split the cache walk until
// M x Hkv x nsplit blocks cover the chip (long contexts of few rows: voice prompts), and the partials are merged by
// attn_combine_rows_kernel.  Returns 0 where attn_wide_kernel ran, else the KV splits of the fall-back (the test hook
// ft_test_wide_attn reports it; the frames ignore it).
template <typename WT, int ROUND>
static int wide_attn(Launch& L, AttnP& a, int li = -1) {
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const int M = L.M, Gq = c.n_head / c.n_local_heads;
    const size_t wlds = (size_t)attn_wide_lds_floats(Gq, c.head_dim, ctx->n_slots) * sizeof(float);
    if (!ctx->no_attn_wide && (long)M * c.n_local_heads >= 128 && c.head_dim == 128 && (Gq == 1 || Gq == 2 || Gq == 4) && wlds <= 65536) {
        a.nsplit = 1;
        const dim3 grid(c.n_local_heads, 1, M);
        if (Gq == 1) attn_wide_kernel<1, 128, WT, ROUND><<<grid, 256, wlds, L.s>>>(a, ctx->n_slots);
        else if (Gq == 2) attn_wide_kernel<2, 128, WT, ROUND><<<grid, 256, wlds, L.s>>>(a, ctx->n_slots);
        else attn_wide_kernel<4, 128, WT, ROUND><<<grid, 256, wlds, L.s>>>(a, ctx->n_slots);
        L.chk();
        if (ctx->trace) tr_rec(L, tr_name("slow.%d.attn", li), M, c.n_head * c.head_dim, TrCls{0}, {TB_XO_Y});
        return 0;
    }
    int ns = 1;
    while (ns < ctx->nsplit && (long)M * c.n_local_heads * ns < 256) ns *= 2;
    a.nsplit = ns;
    a.part_o = ctx->part_o + (size_t)L.m0 * c.n_head * ctx->nsplit * c.head_dim;
    a.part_ml = ctx->part_ml + (size_t)L.m0 * c.n_head * ctx->nsplit * 2;
    attn_decode<WT, ROUND>(L, a);
    if (ctx->trace) {
        if (ns > 1) tr_rec(L, tr_name("slow.%d.attn", li), M, c.n_head * c.head_dim, TrCls{ns}, {TB_PART_O, TB_PART_ML});
        else tr_rec(L, tr_name("slow.%d.attn", li), M, c.n_head * c.head_dim, TrCls{1}, {TB_XO_Y});
    }
    if (ns > 1) {
        attn_combine_rows_kernel<ROUND><<<M, 256, 0, L.s>>>(a); L.chk();
        if (ctx->trace) tr_rec(L, tr_name("slow.%d.attn.merge", li), M, c.n_head * c.head_dim, TrCls{ns}, {TB_XO_Y});
    }
    return ns;
}

// One transformer stack as a decode frame walks it: the slow stack, or the fast stack at one codebook step.  Everything in which
// the two differ only by name is a field; the buffers start at the launch's first row m0.
struct Stack {
    const FtLayer* layers; int n_layer;
    int D, H, Hkv, hd, F, qkvN;
    const float* rope;
    size_t cache_m_stride;      // elements of one slot in a layer's K or V cache
    int nt;                     // GemvP::nt (non-temporal weight loads) of every product of the stack: 1 slow, 0 fast
    int rows;                   // rows of a lock-step Linear: M, or xo_pair + M in the paired pass
    char name[16];              // the launch trace's name of the stack: slow, fast.<cb> or fast.pair (filled while a trace is active)
    RowBuf x, qkv, y, g;        // f32 rows: residual stream, q k v, attention output (stride ctx->y_ld), SwiGLU vector
    XoBuf xo_x, xo_y, xo_g;     // octet-major, lock-step batches: residual stream, attention output, SwiGLU vector
};
static XoBuf xo_at(bf16_t* p, int m0, int id) { return XoBuf{p ? p + (size_t)m0 * 8 : nullptr, id}; }
static Stack slow_stack(const Launch& L) {
    const ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const size_t m0 = L.m0;
    Stack S{ctx->layers.data(), c.n_layer, c.dim, c.n_head, c.n_local_heads, c.head_dim, c.intermediate_size};
    S.qkvN = (S.H + 2 * S.Hkv) * S.hd; S.rope = ctx->rope; S.cache_m_stride = ctx->cache_m_stride; S.nt = 1; S.rows = L.M;
    if (ctx->trace) snprintf(S.name, sizeof S.name, "slow");
    S.x = {ctx->x + m0 * S.D, TB_X}; S.qkv = {ctx->qkv + m0 * S.qkvN, TB_QKV}; S.y = {ctx->y + m0 * ctx->y_ld, TB_Y}; S.g = {ctx->g + m0 * S.F, TB_G};
    S.xo_x = xo_at(ctx->xo_x, L.m0, TB_XO_X); S.xo_y = xo_at(ctx->xo_y, L.m0, TB_XO_Y); S.xo_g = xo_at(ctx->xo_g, L.m0, TB_XO_G);
    return S;
}
// pair: rows [0, M) at position 0 and rows [xo_pair, xo_pair + M) at position 1 (cb == 1) in one pass
static Stack fast_stack(const Launch& L, int cb, bool pair) {
    const ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const size_t m0 = L.m0;
    Stack S{ctx->flayers.data(), c.n_fast_layer, c.fast_dim, c.fast_n_head, c.fast_n_local_heads, c.fast_head_dim, c.fast_intermediate_size};
    S.qkvN = (S.H + 2 * S.Hkv) * S.hd; S.rope = ctx->frope; S.cache_m_stride = ctx->fcache_m_stride; S.nt = 0; S.rows = pair ? ctx->xo_pair + L.M : L.M;
    if (ctx->trace) { if (pair) snprintf(S.name, sizeof S.name, "fast.pair"); else snprintf(S.name, sizeof S.name, "fast.%d", cb); }
    S.x = {ctx->xf + m0 * S.D, TB_XF}; S.qkv = {ctx->qkvf + m0 * S.qkvN, TB_QKVF}; S.g = {ctx->gf + m0 * S.F, TB_GF};
    S.y = {ctx->y + m0 * ctx->y_ld, TB_Y};  // the slow attention's y buffer is free here
    S.xo_x = xo_at(ctx->xo_xf, L.m0, TB_XO_XF); S.xo_y = xo_at(ctx->xo_y, L.m0, TB_XO_Y); S.xo_g = xo_at(ctx->xo_g, L.m0, TB_XO_G);
    return S;
}

// One transformer layer of a decode frame: wqkv, attention, wo, w13, w2, on the GEMV launches or, in a wide batch, on the MFMA
// launches.
//   in, in_xo   the layer's input, which is also the residual of Wo: the stack's own stream, except in layer 0 of the fast
//               stack (the hidden state or a drawn code's embedding); the layer leaves its output in the stack's stream
//   skip_wqkv   the previous draw left this layer's q k v (wide_qkv0_tab): no launch
//   attention   the stack's attention step, (layer, li, Wo's GemvP or null in a wide batch) -> true where it ran Wo itself
// L.gemv_only is the attention step's to honour (no Linear is skipped); S.nt and S.rows are the stack's.
template <typename WT, int ROUND, typename Attn>
static void enqueue_layer(Launch& L, const Stack& S, int li, const float* in, const bf16_t* in_xo, bool skip_wqkv, Attn&& attention) {
    const FtLayer& l = S.layers[li];
    const int HD = S.H * S.hd;
    const auto nm = [&](const char* op) { return TrName{S.name, li, op}; };
    if (wide_batch(L)) {
        if constexpr (ROUND != RND_NONE) {
            // five launches per layer (wide_kernels.h): the residual stream xo, the attention output and the SwiGLU vector
            // travel octet-major in the 16-bit type; q k v stay f32 rows for the attention kernel
            if (!skip_wqkv) wide_linear<WT>(L, nm("wqkv"), in_xo, l.wqkv, l.bqkv_f32, l.attn_norm, S.qkvN, S.D, WEPI_STORE, S.qkv, S.qkvN, XoBuf{}, nullptr, S.rows);
            attention(l, li, nullptr);
            wide_linear<WT>(L, nm("wo"), S.xo_y.p, l.wo, l.bo_f32, nullptr, S.D, HD, WEPI_RESID, RowBuf{}, 0, S.xo_x, in_xo, S.rows);
            wide_linear<WT>(L, nm("w13"), S.xo_x.p, l.w13, nullptr, l.ffn_norm, 2 * S.F, S.D, WEPI_SWIGLU, RowBuf{}, 0, S.xo_g, nullptr, S.rows);
            wide_linear<WT>(L, nm("w2"), S.xo_g.p, l.w2, nullptr, nullptr, S.D, S.F, WEPI_RESID, RowBuf{}, 0, S.xo_x, S.xo_x.p, S.rows);
        }
        return;
    }
    if (!skip_wqkv) gemv_linear<WT, ROUND>(L, nm("wqkv"), l.wqkv, l.bqkv, l.attn_norm, in, S.D, S.qkv, S.qkvN, nullptr, S.qkvN, S.D, EPI_STORE, S.nt);
    const GemvP wo = gemv_params(L.ctx, l.wo, l.bo, nullptr, S.y.p, L.ctx->y_ld, S.x.p, S.D, in, S.D, HD, EPI_RESID, S.nt);
    if (!attention(l, li, &wo)) gemv_launch<WT, ROUND>(L, nm("wo"), S.x.id, wo);
    gemv_linear<WT, ROUND>(L, nm("w13"), l.w13, nullptr, l.ffn_norm, S.x.p, S.D, S.g, S.F, nullptr, 2 * S.F, S.D, EPI_SWIGLU, S.nt);
    gemv_linear<WT, ROUND>(L, nm("w2"), l.w2, nullptr, nullptr, S.g.p, S.F, S.x, S.D, S.x.p, S.D, S.F, EPI_RESID, S.nt);
}

// fast_project_in on the pre-norm hidden state (llama.py:453,590); identity when fast_dim == dim
template <typename WT, int ROUND>
static void enqueue_fproj(Launch& L) {
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    if (c.fast_dim == c.dim) return;
    gemv_linear<WT, ROUND>(L, TrName{nullptr, 0, "fproj"}, ctx->fproj_w, ctx->fproj_b, nullptr, ctx->x + (size_t)L.m0 * c.dim, c.dim,
                           RowBuf{ctx->hid + (size_t)L.m0 * c.fast_dim, TB_HID}, c.fast_dim, nullptr, c.fast_dim, c.dim, EPI_STORE, 0);
}

// One slow-transformer pass over the current input column of rows [m0, m0+M) (llama.py:400-453).
template <typename WT, int ROUND>
static void enqueue_slow(Launch& L, const int* toks, long tok_row_stride, long tok_m_stride, int col, bool with_head) {
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const int m0 = L.m0;
    const Stack S = slow_stack(L);
    const bool wide = wide_batch(L);

    EmbedP e{};
    e.emb = ctx->emb; e.cb_emb = ctx->cb_emb; e.toks = toks; e.tok_row_stride = tok_row_stride;
    e.tok_m_stride = tok_m_stride; e.col = col; e.x = S.x.p; e.ldx = c.dim; e.D = c.dim; e.ncb = c.num_codebooks;
    e.cbsize = c.codebook_size; e.vocab = c.vocab_size; e.sem_begin = c.semantic_begin_id;
    e.sem_end = c.semantic_end_id; e.scale = c.scale_codebook_embeddings;
    e.inv_div = (float)sqrt((double)(c.num_codebooks + 1));
    if (wide) { e.xo = S.xo_x.p; e.xo_ldm = ctx->xo_ldm; }
    if (!L.gemv_only) embed_kernel<WT, ROUND><<<dim3((c.dim + 255) / 256, L.M), 256, 0, L.s>>>(e);
    L.chk();
    if (ctx->trace) { if (wide) tr_rec(L, "embed", L.M, c.dim, TrCls{}, {TB_X, TB_XO_X}); else tr_rec(L, "embed", L.M, c.dim, TrCls{}, {TB_X}); }

    // a wide batch: wide_attn into the octet-major y; 1..4 rows: decode_attn_wo, which also runs Wo (the split merge is inside it)
    auto attention = [&](const FtLayer& l, int li, const GemvP* wo) {
        AttnP a{};
        a.qkv = S.qkv.p; a.ldq = S.qkvN; a.qn = l.qn; a.kn = l.kn; a.rope = S.rope;
        a.kc = (char*)l.kc + (size_t)m0 * S.cache_m_stride * ctx->esz;
        a.vc = (char*)l.vc + (size_t)m0 * S.cache_m_stride * ctx->esz;
        a.cache_m_stride = S.cache_m_stride; a.pos = ctx->d_pos + m0; a.pos_off = L.pos_off;
        a.H = S.H; a.Hkv = S.Hkv; a.hd = S.hd; a.n_slots = ctx->n_slots;
        a.eps = c.norm_eps; a.scale = 1.0f / sqrtf((float)S.hd);
        if (wide) {
            if constexpr (ROUND != RND_NONE) {
                a.y = nullptr; a.ldy = S.H * S.hd; a.y_bf = S.xo_y.p; a.y_xo_ldm = ctx->xo_ldm;
                wide_attn<WT, ROUND>(L, a, li);
            }
            return false;
        }
        a.nsplit = ctx->nsplit; a.y = S.y.p; a.ldy = ctx->y_ld;
        a.part_o = ctx->part_o + (size_t)m0 * S.H * ctx->nsplit * S.hd;
        a.part_ml = ctx->part_ml + (size_t)m0 * S.H * ctx->nsplit * 2;
        decode_attn_wo<WT, ROUND>(L, a, *wo, li);
        return true;
    };
    for (int li = 0; li < S.n_layer; ++li) enqueue_layer<WT, ROUND>(L, S, li, S.x.p, S.xo_x.p, false, attention);
    if (with_head) enqueue_fproj<WT, ROUND>(L);
}

// final norm + vocabulary head (llama.py:446-451); as the slow stack's products it streams its weights with nt = 1
template <typename WT, int ROUND>
static void enqueue_head(Launch& L) {
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const RowBuf logits{ctx->logits + (size_t)L.m0 * c.vocab_size, TB_LOGITS};
    if (wide_batch(L)) {
        if (L.tail_only) {
            xo_from_rows_kernel<WT><<<dim3((c.dim + 255) / 256, L.M), 256, 0, L.s>>>(ctx->x + (size_t)L.m0 * c.dim, c.dim, c.dim,
                                                                             ctx->xo_x + (size_t)L.m0 * 8, ctx->xo_ldm);
            L.chk();
            if (ctx->trace) tr_rec(L, "xo_rows", L.M, c.dim, TrCls{}, {TB_XO_X});
        }
        if constexpr (ROUND != RND_NONE)
            wide_linear<WT>(L, TrName{nullptr, 0, "head"}, ctx->xo_x + (size_t)L.m0 * 8, ctx->head, nullptr, ctx->norm, c.vocab_size, c.dim, WEPI_STORE,
                            logits, c.vocab_size, XoBuf{}, nullptr, 0, true);
        return;
    }
    gemv_linear<WT, ROUND>(L, TrName{nullptr, 0, "head"}, ctx->head, nullptr, ctx->norm, ctx->x + (size_t)L.m0 * c.dim, c.dim, logits, c.vocab_size,
                           nullptr, c.vocab_size, c.dim, EPI_STORE, 1);
}

// Returns what it launched (the test hook ft_test_draw reports it; the frames ignore it): DRAW_* below
enum { DRAW_SMALL = 0, DRAW_BLOCK = 1, DRAW_FOUR = 2, DRAW_PATH_MASK = 3, DRAW_XO_FEMB = 4, DRAW_XO_PAIR = 8, DRAW_QKV0_TAB = 16 };
template <typename WT, int ROUND>
static int enqueue_sample(Launch& L, int cb, bool last) {
    if (L.gemv_only) return -1;
    int what = 0;
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const int m0 = L.m0, R = c.num_codebooks + 1;
    SampP s{};
    if (cb == 0) { s.logits = ctx->logits + (size_t)m0 * c.vocab_size; s.ldl = c.vocab_size; s.V = c.vocab_size; }
    else { s.logits = ctx->flog + (size_t)m0 * ctx->fastV; s.ldl = ctx->fastV; s.V = ctx->fastV; }
    s.ctl = ctx->d_ctl + m0; s.tokn = ctx->d_tokn + (size_t)m0 * R; s.seq = ctx->d_seq + (size_t)m0 * R * ctx->cap;
    s.cap = ctx->cap; s.nf = ctx->d_nf + m0; s.cb = cb; s.ncb = c.num_codebooks; s.sem_begin = c.semantic_begin_id;
    s.im_end = c.im_end_id; s.cbsize = c.codebook_size; s.fast_emb = ctx->fast_emb;
    s.femb = ctx->femb + (size_t)m0 * c.fast_dim; s.Df = c.fast_dim; s.noise = ctx->noise;
    s.noise_row_len = ctx->noise_row_len; s.noise_rows = ctx->noise_rows;
    s.noise_off = cb == 0 ? 0 : (long)c.vocab_size + (long)(cb - 1) * ctx->fastV;
    s.last = last ? 1 : 0; s.tok = ctx->d_tok + (size_t)m0 * R; s.pos = ctx->d_pos + m0; s.done = ctx->d_done + m0;
    if (wide_batch(L)) {
        // the semantic code's embedding is position 1 of the paired pass: it joins the slow stack's residual stream
        s.femb_xo = (cb == 0 && wide_pair(L) ? ctx->xo_x + (size_t)ctx->xo_pair * 8 : ctx->xo_femb) + (size_t)m0 * 8;
        s.femb_ldm = ctx->xo_ldm;
        what |= cb == 0 && wide_pair(L) ? DRAW_XO_PAIR : DRAW_XO_FEMB;
        if (cb >= 1 && cb + 1 < c.num_codebooks && ctx->wide_qkv0_tab) {     // the next codebook step's layer-0 q k v (its launch is skipped)
            what |= DRAW_QKV0_TAB;
            s.qkv0_tab = ctx->wide_qkv0_tab; s.qkv0_n = (c.fast_n_head + 2 * c.fast_n_local_heads) * c.fast_head_dim;
            s.qkv0_out = ctx->qkvf + (size_t)m0 * s.qkv0_n;
        }
    }
    // what a finishing draw launch may write (finish_draw): the frame under construction and, on the last codebook, the state
    auto tr_draw = [&](const char* sfx, int w) {
        const std::string nm = tr_name("draw.%d%s", cb, sfx);
        if (!wide_batch(L)) tr_rec(L, nm, L.M, s.V, TrCls{w}, {cb == 0 ? TB_LOGITS : TB_FLOG, TB_TOKN, TB_TOK, TB_POS, TB_NF, TB_DONE, TB_SEQ, TB_FEMB});
        else tr_rec(L, nm, L.M, s.V, TrCls{w}, {cb == 0 ? TB_LOGITS : TB_FLOG, TB_TOKN, TB_TOK, TB_POS, TB_NF, TB_DONE, TB_SEQ, TB_FEMB, TB_XO_FEMB, TB_XO_X, TB_QKVF});
    };
    if (s.V <= 1024) {
        sample_small_kernel<WT, ROUND><<<L.M, 256, 0, L.s>>>(s);
        what |= DRAW_SMALL;
        if (ctx->trace) tr_draw("", what);
    } else if (ROUND == RND_BF16) {
        // large vocabulary, bf16: the histogram of the 65 536 bf16 classes and the search of the top-p cut on it in ONE block
        // per row (LDS counters), then index-ordered tie handling and the chip-wide race
        SampBigP b{};
        b.s = s; b.nchunk = (s.V + 1023) / 1024;
        b.cut = ctx->samp_cut + m0;
        b.chunk_cnt = ctx->samp_chunk_cnt + (size_t)m0 * b.nchunk;
        b.part_score = ctx->samp_part_score + (size_t)m0 * b.nchunk;
        b.part_idx = ctx->samp_part_idx + (size_t)m0 * b.nchunk;
        const dim3 gridc(b.nchunk, L.M);
        {
            static DevOnce once;     // per device
            once.run([] {
                hipFuncSetAttribute((const void*)samp_cut_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SAMP_TH_LDS);
            });
        }
        what |= DRAW_FOUR;
        samp_cut_kernel<<<L.M, SAMP_TH_THREADS, SAMP_TH_LDS, L.s>>>(b);
        if (ctx->trace) tr_rec(L, tr_name("draw.%d.cut", cb), L.M, s.V, TrCls{what}, {TB_LOGITS, TB_CUT});
        samp_count_kernel<<<gridc, 256, 0, L.s>>>(b);
        if (ctx->trace) tr_rec(L, tr_name("draw.%d.count", cb), L.M, s.V, TrCls{what}, {TB_CUT, TB_CHUNK_CNT});
        samp_race_kernel<<<gridc, 256, 0, L.s>>>(b);
        if (ctx->trace) tr_rec(L, tr_name("draw.%d.race", cb), L.M, s.V, TrCls{what}, {TB_PART_IDX});
        samp_finish_kernel<WT><<<L.M, 256, 0, L.s>>>(b);
        if (ctx->trace) tr_draw(".finish", what);
    } else {
        sample_block_kernel<WT, ROUND><<<L.M, 1024, 0, L.s>>>(s);
        what |= DRAW_BLOCK;
        if (ctx->trace) tr_draw("", what);
    }
    L.chk();
    return what;
}

// The fast transformer over codebook positions 0..ncb-1 with its sampling (inference.py:115-149).
template <typename WT, int ROUND>
static void enqueue_fast_step(Launch& L, const int cb, const bool pair = false) {
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const int m0 = L.m0, M = L.M;
    const Stack S = fast_stack(L, cb, pair);
    const bool wide = wide_batch(L);
    // layer 0 reads the slow stack's hidden state (position 0; in a wide batch its residual stream) or the drawn code's
    // embedding; the paired pass reads both from the slow stack's stream, where the semantic draw left position 1's rows
    const float* xin = cb == 0 ? ctx->hid + (size_t)m0 * S.D : ctx->femb + (size_t)m0 * S.D;
    const bf16_t* xin_o = wide ? ((cb == 0 || pair) ? ctx->xo_x : ctx->xo_femb) + (size_t)m0 * 8 : nullptr;

    auto attention = [&](const FtLayer& l, int li, const GemvP*) {
        FastAttnP a{};
        a.qkv = S.qkv.p; a.ldq = S.qkvN; a.qn = l.qn; a.kn = l.kn; a.rope = S.rope;
        a.kc = (char*)l.kc + (size_t)m0 * S.cache_m_stride * ctx->esz;
        a.vc = (char*)l.vc + (size_t)m0 * S.cache_m_stride * ctx->esz;
        a.cache_m_stride = S.cache_m_stride; a.H = S.H; a.Hkv = S.Hkv; a.hd = S.hd;
        a.ncb = c.num_codebooks; a.eps = c.norm_eps; a.scale = (float)(1.0 / sqrt((double)S.hd));
        const int HD = S.H * S.hd, rows = pair ? 2 * M : M;      // (a paired pass is a wide batch)
        if (wide) {
            a.c = pair ? 0 : cb; a.y_bf = S.xo_y.p; a.y_xo_ldm = ctx->xo_ldm;
            a.pair_M = pair ? M : 0; a.pair_off = ctx->xo_pair;
            fast_attn_kernel<WT, ROUND><<<dim3(S.H, rows), 64, 0, L.s>>>(a, nullptr, HD);
        } else {
            a.c = cb;
            if (!L.gemv_only) fast_attn_kernel<WT, ROUND><<<dim3(S.H, rows), 64, 0, L.s>>>(a, S.y.p, ctx->y_ld);
        }
        L.chk();
        if (ctx->trace) tr_rec(L, TrName{S.name, li, "attn"}.str(), rows, HD, TrCls{}, {wide ? S.xo_y.id : S.y.id});
        return false;
    };
    for (int li = 0; li < S.n_layer; ++li) {
        // layer 0 of steps >= 2: the draw of the previous step left this step's q k v (wide_qkv0_build)
        const bool tab = wide && li == 0 && cb >= 2 && !pair && ctx->wide_qkv0_tab;
        enqueue_layer<WT, ROUND>(L, S, li, li == 0 ? xin : S.x.p, li == 0 ? xin_o : S.xo_x.p, tab, attention);
    }
    if (cb == 0) return;  // logits of position 0 are discarded (inference.py:122)
    const TrName head{"fast", cb, "head"};
    const RowBuf flog{ctx->flog + (size_t)m0 * ctx->fastV, TB_FLOG};
    if (wide) {
        if constexpr (ROUND != RND_NONE)
            wide_linear<WT>(L, head, (S.n_layer > 0 ? ctx->xo_xf : ctx->xo_femb) + (size_t)(m0 + (pair ? ctx->xo_pair : 0)) * 8, ctx->fast_out, nullptr,
                            ctx->fast_norm, ctx->fastV, S.D, WEPI_STORE, flog, ctx->fastV, XoBuf{}, nullptr);
    } else {
        gemv_linear<WT, ROUND>(L, head, ctx->fast_out, nullptr, ctx->fast_norm, S.x.p, S.D, flog, ctx->fastV, nullptr, ctx->fastV, S.D, EPI_STORE, S.nt);
    }
    enqueue_sample<WT, ROUND>(L, cb, cb == c.num_codebooks - 1);
}

// everything after the slow layers: vocabulary head, semantic draw, the fast codebooks
template <typename WT, int ROUND>
static void enqueue_frame_tail(Launch& L) {
    ft_ctx* ctx = L.ctx;
    const int ncb = ctx->c.num_codebooks;
    enqueue_head<WT, ROUND>(L);
    if (L.gemv_only) return;  // measurement graph: the HBM-streamed launches only (slow layers above + the head)
    enqueue_sample<WT, ROUND>(L, 0, ncb == 1);
    if (ROUND == RND_BF16 && eng_fast_ok(L)) { enqueue_fast_engine(L); return; }
    int cb0 = 0;
    if (wide_pair(L)) { enqueue_fast_step<WT, ROUND>(L, 1, true); cb0 = 2; }
    for (int cb = cb0; cb < ncb; ++cb) enqueue_fast_step<WT, ROUND>(L, cb);
}

// One full frame: slow pass on the current column, semantic sample, fast codebooks (inference.py:83-155).
template <typename WT, int ROUND>
static void enqueue_frame_t(Launch& L, const int* toks, long trs, long tms, int col) {
    if (ROUND == RND_BF16 && eng_slow_ok(L)) enqueue_slow_engine(L, toks, trs, tms, col);
    else enqueue_slow<WT, ROUND>(L, toks, trs, tms, col, true);
    enqueue_frame_tail<WT, ROUND>(L);
}

static void enqueue_frame(Launch& L, const int* toks, long trs, long tms, int col) {
    by_dtype(L.ctx, [&](auto t) { using T = decltype(t); enqueue_frame_t<typename T::WT, T::ROUND>(L, toks, trs, tms, col); });
}
static void enqueue_slow_only(Launch& L, const int* toks, long trs, long tms, int col) {
    by_dtype(L.ctx, [&](auto t) { using T = decltype(t); enqueue_slow<typename T::WT, T::ROUND>(L, toks, trs, tms, col, false); });
}
// the frame tail after a prompt pass, whose last position left the rows' hidden state in ctx->x
static void enqueue_tail(Launch& L) {
    by_dtype(L.ctx, [&](auto t) { using T = decltype(t); enqueue_fproj<typename T::WT, T::ROUND>(L); enqueue_frame_tail<typename T::WT, T::ROUND>(L); });
}

// ------------------------------------------------------------------------------------------ AR API
static ft_status eng_recover(ft_ctx* ctx, bool* aborted);
static bool eng_in_use(const ft_ctx* ctx);
// Frames that ran on the frame engine must not pass where one of its hand-offs timed out: once the stream has drained,
// eng_recover tells; then `rewind` puts the slot back where those frames began and `rerun` enqueues them again on the launch
// path (ctx->eng_suspended).
template <typename Rewind, typename Rerun>
static ft_status eng_fallback(ft_ctx* ctx, Rewind&& rewind, Rerun&& rerun) {
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    bool aborted = false;
    FT_TRY(eng_recover(ctx, &aborted));
    if (!aborted) return FT_OK;
    FT_TRY(rewind());
    ctx->eng_suspended = true;
    const ft_status st = rerun();
    ctx->eng_suspended = false;
    return st;
}
static ft_status ar_ready(ft_ctx* ctx) {
    if (!ctx) return FT_ERR_ARG;
    if (!ctx->has_ar) return ft_fail(ctx, FT_ERR_STATE, "context was created without an AR config");
    if (!ctx->finalized) return ft_fail(ctx, FT_ERR_STATE, "weights not finalized (ft_finalize_weights)");
    if (hipSetDevice(ctx->device) != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "hipSetDevice failed");
    return FT_OK;
}

extern "C" ft_status ft_ar_reset(ft_ctx* ctx, int32_t slot) {
    if (!ctx || !ctx->has_ar) return FT_ERR_ARG;
    if (slot < 0 || slot >= ctx->c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_reset: bad slot");
    FT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t R = ctx->c.num_codebooks + 1;
    FT_HIP(ctx, hipMemsetAsync(ctx->d_seq + (size_t)slot * R * ctx->cap, 0, R * ctx->cap * sizeof(int), ctx->stream));
    FT_HIP(ctx, hipMemsetAsync(ctx->d_pos + slot, 0, sizeof(int), ctx->stream));
    FT_HIP(ctx, hipMemsetAsync(ctx->d_nf + slot, 0, sizeof(int), ctx->stream));
    FT_HIP(ctx, hipMemsetAsync(ctx->d_done + slot, 0, sizeof(int), ctx->stream));
    return FT_OK;
}

// KV splits of the decode attention for a call whose longest context ends at pos_end (more blocks walking the cache in
// parallel); measured at s1-mini shapes (tools/longctx_probe.py): 8 splits are fastest up to ~700 positions, 16 up to ~3000
static void pick_nsplit(ft_ctx* ctx, int pos_end) {
    if (ctx->nsplit_fixed || ctx->nsplit_max <= 1) return;
    const int want = pos_end <= 768 ? 8 : pos_end <= 3072 ? 16 : 32;
    ctx->nsplit = std::min(want, ctx->nsplit_max);
}

static ft_status upload_ctl(ft_ctx* ctx, int m0, int n, const ft_sampling* sp) {
    std::vector<RowCtl> h(n);
    for (int i = 0; i < n; ++i) {
        h[i].temperature = sp[i].temperature; h[i].top_p = sp[i].top_p; h[i].rep = sp[i].repetition_penalty;
        h[i].ban_eos = sp[i].ban_eos; h[i].seed = sp[i].seed;
    }
    FT_HIP(ctx, hipMemcpyAsync(ctx->d_ctl + m0, h.data(), n * sizeof(RowCtl), hipMemcpyHostToDevice, ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // h goes out of scope
    return FT_OK;
}

// MFMA prefill (bf16 precision): the whole prompt goes through every slow layer as S = Lp rows on the
template <int HD, int NG>
static void flash_launch(const FlashP& fp, int Lp, hipStream_t st, int nz = 1) {
    constexpr size_t lds = flash_prefill_lds<HD, NG>();
    static DevOnce once;
    once.run([] { hipFuncSetAttribute((const void*)flash_prefill_kernel<HD, NG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
    constexpr int QROWS = 16 * (8 / NG);
    flash_prefill_kernel<HD, NG><<<dim3(fp.H, (Lp + QROWS - 1) / QROWS, nz), 512, lds, st>>>(fp);
}

template <int BM, int BN, int NWM, int NWN, int DEPTH = 4, int MINW = 1>
static void lingemm_launch(const TapGemmP& p, int S, int N, hipStream_t st) {
    constexpr size_t lds = lingemm_lds_bytes<BM, BN, NWM>();
    static DevOnce once;     // per device: the dynamic-LDS opt-in belongs to the device's function object
    once.run([] { hipFuncSetAttribute((const void*)lingemm_kernel<BM, BN, NWM, NWN, DEPTH, MINW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
    lingemm_kernel<BM, BN, NWM, NWN, DEPTH, MINW><<<dim3((S + BM - 1) / BM, N / BN), 64 * NWM * NWN, lds, st>>>(p);
}

// tap-GEMM kernel (v_mfma_f32_16x16x32_bf16), with the reference's rounding points in the epilogues
// (Linear output rounded, residual add rounded, SwiGLU steps rounded; llama.py:172-190,229-283,322-331).
// K/V of all positions are appended first, then every position attends over the cache.
// The choice between the kernel classes below is checked ONE LAUNCH AT A TIME through this very dispatcher: ft_test_pf_linear
// runs one product of each of prefill_gemm's four forms on temporaries, and tests/test_pf_kernels_gpu.py compares every
// element of every written row with the float64 restatement of tests/pf_ref.py (every class, both sides of every row-tile
// and K-round edge, the in-place residual form included).
static int pf_gemm(Launch& L, const bf16_t* X, long ldx, int S, const void* W, const float* bias, int N, int K,
                   int act, const float* resid, float* out_f32, bf16_t* out_bf, long ldo, int round_out, const PfX& fx) {
    int id = PF_ID_NONE;
    TapGemmP p{};
    p.gain = (const bf16_t*)fx.gain; p.ss_in = fx.ss_in; p.ss_out = fx.ss_out; p.ss_nblk = fx.nblk;
    p.ss_ld = std::max(L.ctx->c.dim, L.ctx->c.fast_dim) / 16 + 1; p.eps = L.ctx->c.norm_eps;
    p.X = X; p.ldx = ldx; p.T_in = S; p.W = (const bf16_t*)W; p.ntap = 1; p.offs[0] = 0; p.M = S; p.N = N; p.K = K;
    p.bias = bias; p.n_mod = N; p.act = act; p.resid_f32 = resid; p.ldr = ldo; p.out_f32 = out_f32; p.out_bf = out_bf;
    p.ldo = ldo; p.round_lin = 1; p.round_f32_out = round_out;
    const int mode = L.ctx->prefill_gemm_mode;  // FT_PREFILL_GEMM: 0 = first tile kernel only, 1 = no skinny kernel
    const bool fused = fx.gain || fx.ss_out;
    if ((mode >= 2 || fused) && S <= 128 && K % 128 == 0 && N % 2 == 0) {
        // short prompts are weight-bandwidth bound: 16 weight rows per block, K split over the waves
        if (S <= 16) { id = PF_ID_SKINNY1; skinny_gemm_launch<1>(p, 1, L.s); }
        else if (S <= 32) { id = PF_ID_SKINNY2; skinny_gemm_launch<2>(p, 1, L.s); }
        else { id = PF_ID_SKINNY4; skinny_gemm_launch<4>(p, (S + 63) / 64, L.s); }
    } else if (fused) {
        L.err = hipErrorInvalidValue;   // the fused norm exists on the skinny kernel only (callers check the shapes)
    } else if (mode >= 1 && K % 64 == 0 && N % 128 == 0) {
        // long prompts (reference audio): MFMA tiles with four K-steps of both operands in flight (lingemm_kernel) - 128 x 128
        // on 8 waves for the wide products from 512 rows, 64 x 64 on 4 waves otherwise (the N = 1024 products would leave
        // 200 CUs idle on the large tile: 56 workgroups at 780 rows).  Measured at 780 rows (tools/prefill_probe.py): 7.05 ms
        // with the codec's one-step-ahead tile kernel, 4.89 ms with these (3.50 against 5.61 ms at 256 rows).
        constexpr int tile8_s = 512;
        if (K % 256 == 0) {
            // both tiles are held to <= 128 registers so that workgroups share a CU (128 x 128: two K-steps in flight, two
            // workgroups per CU - 4.92 against 5.25 ms per 780-position prefill with four steps and one workgroup; 64 x 64: four
            // steps, four workgroups - another 0.07 ms)
            if (S >= tile8_s && N > 1024) { id = PF_ID_LIN128; lingemm_launch<128, 128, 2, 4, 2, 4>(p, S, N, L.s); }
            else { id = PF_ID_LIN64; lingemm_launch<64, 64, 2, 2, 4, 4>(p, S, N, L.s); }
        } else if (S >= tile8_s) {
            id = PF_ID_TAP64_128;
            constexpr size_t lds8 = std::max((size_t)((128 + 56) + 2 * 128) * (64 + 8) * 2, (size_t)(128 / 2) * (128 + 4) * 4);
            static DevOnce once8;
            once8.run([] { hipFuncSetAttribute((const void*)tapgemm64_kernel<128, 128, 64, 2, 4>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds8); });
            tapgemm64_kernel<128, 128, 64, 2, 4><<<dim3((S + 127) / 128, N / 128, 1), 512, lds8, L.s>>>(p);
        } else {
            id = PF_ID_TAP64_64;
            const size_t lds = std::max((size_t)((64 + 56) + 2 * 64) * (64 + 8) * 2, (size_t)(64 / 2) * (64 + 4) * 4);
            tapgemm64_kernel<64, 64, 64><<<dim3((S + 63) / 64, N / 64, 1), 256, lds, L.s>>>(p);
        }
    } else if (N >= 128) { id = PF_ID_TAP_128; tapgemm_kernel<128, 128, 2, 2><<<dim3((S + 127) / 128, (N + 127) / 128, 1), 256, 0, L.s>>>(p); }
    else { id = PF_ID_TAP_64; tapgemm_kernel<128, 64, 4, 1><<<dim3((S + 127) / 128, (N + 63) / 64, 1), 256, 0, L.s>>>(p); }
    L.chk();
    return id;
}

// rg: the rows are the prompts of rg->n slots back to back (ctx->pf_seqs / pf_rows describe them; Lp = all rows, slot and
// pos0 unused): the Linear products and norms do not care, the K/V append and the attention go by sequence.
struct RaggedPf { int n, max_lp; };
static __global__ __launch_bounds__(256) void gather_last_rows_kernel(const float* pf_x, int D, const int4* seqs, float* x) {
    const int4 sq = seqs[blockIdx.x];
    for (int d = threadIdx.x; d < D; d += 256) x[(size_t)sq.w * D + d] = pf_x[(size_t)(sq.x + sq.y - 1) * D + d];
}
// The attention of one layer of a prompt pass: the K/V append of every row, then the causal attention.  Three choices live
// here: the tiled kernel or the decode kernel position by position, its NG key groups, its head width.  prefill_gemm calls it
// on the context's workspace and ft_test_pf_attn on temporaries (tests/test_pf_kernels_gpu.py: y, the finished queries and
// the appended rows of ONE such pass against the float64 restatement of tests/pf_ref.py, every other cache row bit-unchanged).
// kc / vc: the layer's base pointers (slot 0).  Returns the path taken: NG of flash_prefill_kernel, 0 = position by position.
struct PfAttnIO {
    const float* qkv;          // [rows][(H + 2 Hkv) hd]
    const void *qn, *kn;
    void *kc, *vc;
    float* y;                  // [rows][H hd] f32 (the per-position kernel writes it too)
    bf16_t* y_bf;              // [rows][H hd]
    bf16_t* q_bf;              // [rows][H hd]: the finished queries (tiled path only)
    const int4* seqs;          // ragged pass: device copies of {first row, rows, first cache position, slot} per sequence ...
    const int2* rows;          // ... and of (slot, cache position) per row
};
// li: the layer, for the launch trace's names (pf.<li>.append, pf.<li>.attn; class {1 tiled | 0} and {the path})
static int pf_attn(Launch& L, const PfAttnIO& io, int slot, int Lp, int pos0, const RaggedPf* rg, int li = -1) {
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const int HD = c.n_head * c.head_dim, qkvN = (c.n_head + 2 * c.n_local_heads) * c.head_dim;
    const int G = c.n_head / c.n_local_heads;
    const int nslot = 2048 / c.head_dim;
    const size_t lds = ((size_t)G * c.head_dim + 2 * c.head_dim + (size_t)nslot * G * 2 + (size_t)nslot * G * c.head_dim) * sizeof(float);
    int path = 0;
    AttnP a{};
    a.qkv = io.qkv; a.ldq = qkvN; a.qn = io.qn; a.kn = io.kn; a.rope = ctx->rope;
    a.kc = (char*)io.kc + (size_t)slot * ctx->cache_m_stride * ctx->esz;
    a.vc = (char*)io.vc + (size_t)slot * ctx->cache_m_stride * ctx->esz;
    a.cache_m_stride = 0; a.pos = nullptr; a.pos_off = pos0; a.row_is_pos = 1;
    if (rg) { a.kc = io.kc; a.vc = io.vc; a.cache_m_stride = ctx->cache_m_stride; a.row_sp = io.rows; }
    a.H = c.n_head; a.Hkv = c.n_local_heads; a.hd = c.head_dim; a.n_slots = ctx->n_slots; a.nsplit = 1;
    a.eps = c.norm_eps; a.scale = 1.0f / sqrtf((float)c.head_dim); a.y = io.y; a.ldy = HD; a.y_bf = io.y_bf;
    // pass 0 appends K/V of every position (and leaves the finished queries); pass 1 attends: on the matrix cores
    // for 64- and 128-wide heads, otherwise position by position with the decode kernel
    // (a short tail behind a long restored prefix: with four key groups per block the tiled kernel wins from 16 new
    // positions - 47.7 against 49.5 ms to the first 10 frames of 8 cloned-voice utterances with 49-token tails; round 2's
    // one-group kernel lost below 64)
    const bool flash = rg || (!getenv("FT_PREFILL_ATTN_V0") && (c.head_dim == 64 || c.head_dim == 128) && Lp >= 16);
    a.q_out = flash ? io.q_bf : nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        a.kv_only = pass == 0; a.no_append = pass == 1;
        if (pass == 0 && flash) {       // every position's q k v in one launch of Lp blocks
            if (c.head_dim == 128) prefill_rope_append_kernel<128><<<Lp, 256, 0, L.s>>>(a);
            else prefill_rope_append_kernel<64><<<Lp, 256, 0, L.s>>>(a);
            L.chk();
            if (ctx->trace) tr_rec(L, tr_name("pf.%d.append", li), Lp, HD, TrCls{1}, {TB_PF_QBF});
            continue;
        }
        if (pass == 1 && flash) {
            FlashP fp{io.q_bf, (const bf16_t*)a.kc, (const bf16_t*)a.vc, io.y_bf, Lp, c.n_head, c.n_local_heads,
                      c.head_dim, ctx->n_slots, pos0, a.scale};
            int nz = 1, lp_grid = Lp;
            if (rg) { fp.seqs = io.seqs; fp.cache_m_stride = ctx->cache_m_stride; nz = rg->n; lp_grid = rg->max_lp; }
            // key groups per block: four (32 query rows per block: more blocks) up to 320 positions, two beyond (measured:
            // 3.39 against 3.46 ms per 160-position prefill, 5.24 against 4.91 at 780 - the longer walks re-read K/V twice as often)
            const bool ng4 = lp_grid <= 320;
            path = ng4 ? 4 : 2;
            if (c.head_dim == 128) { if (ng4) flash_launch<128, 4>(fp, lp_grid, L.s, nz); else flash_launch<128, 2>(fp, lp_grid, L.s, nz); }
            else { if (ng4) flash_launch<64, 4>(fp, lp_grid, L.s, nz); else flash_launch<64, 2>(fp, lp_grid, L.s, nz); }
            L.chk();
            if (ctx->trace) tr_rec(L, tr_name("pf.%d.attn", li), Lp, HD, TrCls{path}, {TB_PF_YBF});
            continue;
        }
        const dim3 grid(c.n_local_heads, 1, Lp);
        switch (G) {
            case 1: attn_decode_kernel<bf16_t, 1, true><<<grid, 256, lds, L.s>>>(a); break;
            case 2: attn_decode_kernel<bf16_t, 2, true><<<grid, 256, lds, L.s>>>(a); break;
            case 4: attn_decode_kernel<bf16_t, 4, true><<<grid, 256, lds, L.s>>>(a); break;
            default:
                hipFuncSetAttribute((const void*)attn_decode_kernel<bf16_t, 8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                attn_decode_kernel<bf16_t, 8, true><<<grid, 256, lds, L.s>>>(a);
        }
        L.chk();
        if (ctx->trace) {
            if (pass == 0) tr_rec(L, tr_name("pf.%d.append", li), Lp, HD, TrCls{0}, {TB_PF_QBF});
            else tr_rec(L, tr_name("pf.%d.attn", li), Lp, HD, TrCls{0}, {TB_PF_Y, TB_PF_YBF});
        }
    }
    return path;
}
static void prefill_gemm(Launch& L, int slot, int Lp, int pos0, bool with_tail = true, const RaggedPf* rg = nullptr) {
    ft_ctx* ctx = L.ctx;
    const ft_ar_config& c = ctx->c;
    const int D = c.dim, HD = c.n_head * c.head_dim, F = c.intermediate_size;
    const int qkvN = (c.n_head + 2 * c.n_local_heads) * c.head_dim;
    EmbedP e{};
    e.emb = ctx->emb; e.cb_emb = ctx->cb_emb; e.toks = ctx->d_prompt; e.tok_row_stride = Lp; e.tok_m_stride = 1;
    e.col = 0; e.x = ctx->pf_x; e.ldx = D; e.D = D; e.ncb = c.num_codebooks; e.cbsize = c.codebook_size;
    e.vocab = c.vocab_size; e.sem_begin = c.semantic_begin_id; e.sem_end = c.semantic_end_id;
    e.scale = c.scale_codebook_embeddings; e.inv_div = (float)sqrt((double)(c.num_codebooks + 1));
    embed_kernel<bf16_t, true><<<dim3((D + 255) / 256, Lp), 256, 0, L.s>>>(e);
    L.chk();
    // the launch trace's records (fishtts_hip_test.h): pf.embed, pf.<l>.<op>, pf.last; a product's class is pf_gemm's PF_ID_*
    const auto rec = [&](const char* op, int li, int cols, int id, int buf) {
        if (ctx->trace) tr_rec(L, li < 0 ? tr_name("pf.%s", op) : tr_name("pf.%d.%s", li, op), Lp, cols, TrCls{id}, {buf});
    };
    rec("embed", -1, D, -1, TB_PF_X);
    for (int li = 0; li < c.n_layer; ++li) {
        const FtLayer& l = ctx->layers[li];
        rmsnorm_llama_rows_kernel<bf16_t, true><<<Lp, 256, 0, L.s>>>(ctx->pf_x, l.attn_norm, c.norm_eps, D, ctx->pf_xn);
        rec("norm1", li, D, -1, TB_PF_XN);
        rec("wqkv", li, qkvN, pf_gemm(L, ctx->pf_xn, D, Lp, l.wqkv, l.bqkv_f32, qkvN, D, ACT_NONE, nullptr, ctx->pf_qkv, nullptr, qkvN, 0), TB_PF_QKV);
        PfAttnIO io{ctx->pf_qkv, l.qn, l.kn, l.kc, l.vc, ctx->pf_y, ctx->pf_ybf, ctx->pf_qbf, ctx->pf_seqs, ctx->pf_rows};
        pf_attn(L, io, slot, Lp, pos0, rg, li);
        rec("wo", li, D, pf_gemm(L, ctx->pf_ybf, HD, Lp, l.wo, l.bo_f32, D, HD, ACT_NONE, ctx->pf_x, ctx->pf_x, nullptr, D, 1), TB_PF_X);
        rmsnorm_llama_rows_kernel<bf16_t, true><<<Lp, 256, 0, L.s>>>(ctx->pf_x, l.ffn_norm, c.norm_eps, D, ctx->pf_xn);
        rec("norm2", li, D, -1, TB_PF_XN);
        rec("w13", li, F, pf_gemm(L, ctx->pf_xn, D, Lp, l.w13, nullptr, 2 * F, D, ACT_SWIGLU, nullptr, nullptr, ctx->pf_g, F, 0), TB_PF_G);
        rec("w2", li, D, pf_gemm(L, ctx->pf_g, F, Lp, l.w2, nullptr, D, F, ACT_NONE, ctx->pf_x, ctx->pf_x, nullptr, D, 1), TB_PF_X);
    }
    // the last position feeds the head and the fast stack through the decode kernels
    if (rg) {
        gather_last_rows_kernel<<<rg->n, 256, 0, L.s>>>(ctx->pf_x, D, ctx->pf_seqs, ctx->x); L.chk();
        if (ctx->trace) tr_rec(L, "pf.last", rg->n, D, TrCls{}, {TB_X});
        return;
    }
    hipMemcpyAsync(ctx->x + (size_t)slot * D, ctx->pf_x + (size_t)(Lp - 1) * D, D * sizeof(float), hipMemcpyDeviceToDevice, L.s);
    if (ctx->trace) tr_rec(L, "pf.last", 1, D, TrCls{}, {TB_X});
    if (!with_tail) return;   // ft_ar_prefill_slow: the first frames of several slots are drawn together later
    enqueue_fproj<bf16_t, true>(L);
    enqueue_frame_tail<bf16_t, true>(L);
}

extern "C" ft_status ft_ar_prefill_at(ft_ctx* ctx, int32_t slot, const int32_t* prompt, int32_t Lp, int32_t pos0,
                                      const ft_sampling* sp, int32_t* out_frame) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (!prompt || !sp || !out_frame) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill: null argument");
    if (slot < 0 || slot >= c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill: bad slot");
    if (Lp < 1) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill: empty prompt");
    if (pos0 < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill_at: pos0 < 0");
    if (pos0 + Lp >= c.max_seq_len) {  // inference.py:296-299
        char buf[128];
        snprintf(buf, sizeof buf, "Input sequence length %d exceeds max_seq_len %d", pos0 + Lp, c.max_seq_len);
        return ft_fail(ctx, FT_ERR_TOO_LONG, buf);
    }
    const int R = c.num_codebooks + 1;
    const bool on_engine = eng_in_use(ctx);
    if (ctx->tstore.armed && on_engine) {
        ctx->tstore.armed = false;
        return ft_fail(ctx, FT_ERR_STATE, "ft_ar_prefill: a traced call never runs on the frame engine");
    }
    ArTraceScope traced(ctx, true, 3, slot, 1);
    if (traced.own) tr_state(ctx, 0);  // before the reset: what it does to the slot is part of the record
    ctx->hid_in_xo[slot] = 0;
    FT_TRY(ft_ar_reset(ctx, slot));
    FT_TRY(upload_ctl(ctx, slot, 1, sp));
    FT_HIP(ctx, hipMemcpyAsync(ctx->d_prompt, prompt, (size_t)R * Lp * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    tr_uploaded(ctx, {TB_PROMPT});
    pick_nsplit(ctx, pos0 + Lp);       // (position-by-position prompt passes: the split count of this prompt's length)
    Launch L{ctx, ctx->stream, slot, 1, 0};
    if (!ctx->prefill_v0) {
        prefill_gemm(L, slot, Lp, pos0);
    } else {
        // f32 precision (and shapes the MFMA tiles do not cover): the prompt is fed through the S=1 decode
        // kernels position by position (same causal arithmetic); only the last position runs the head
        for (int t = 0; t < Lp - 1; ++t) {
            L.pos_off = pos0 + t;
            tr_pos(ctx, t);
            enqueue_slow_only(L, ctx->d_prompt, Lp, 0, t);
        }
        L.pos_off = pos0 + Lp - 1;
        tr_pos(ctx, Lp - 1);
        enqueue_frame(L, ctx->d_prompt, Lp, 0, Lp - 1);
    }
    if (L.err != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("prefill launch: ") + hipGetErrorString(L.err));
    if (on_engine) {
        // the first frame's codebook loop (and, position by position, its slow pass) ran on the frame engine: a hand-off
        // time-out there must not pass for a first frame - redo that frame on the launch path (the prompt's K/V and the
        // last position's hidden state are untouched by it)
        FT_TRY(eng_fallback(ctx, [&] { return ft_ar_reset(ctx, slot); }, [&]() -> ft_status {
            if (!ctx->prefill_v0) enqueue_tail(L);      // (the MFMA prompt pass is bf16 only)
            else enqueue_frame(L, ctx->d_prompt, Lp, 0, Lp - 1);
            return L.err == hipSuccess ? FT_OK : ft_fail(ctx, FT_ERR_HIP, std::string("prefill launch: ") + hipGetErrorString(L.err));
        }));
    }
    // finalize() advanced pos 0 -> 1; the next input position is pos0 + Lp
    ctx->h_pin[0] = pos0 + Lp;
    FT_HIP(ctx, hipMemcpyAsync(ctx->d_pos + slot, ctx->h_pin, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FT_HIP(ctx, hipMemcpyAsync(out_frame, ctx->d_tok + (size_t)slot * R, R * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (traced.own) tr_state(ctx, 1);
    return FT_OK;
}

// Prompt pass without the first frame: K/V of the prompt and the last position's hidden state stay on the device.
extern "C" ft_status ft_ar_prefill_slow(ft_ctx* ctx, int32_t slot, const int32_t* prompt, int32_t Lp, int32_t pos0) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (!prompt) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill_slow: null argument");
    if (slot < 0 || slot >= c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill_slow: bad slot");
    if (Lp < 1 || pos0 < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill_slow: empty prompt");
    if (pos0 + Lp >= c.max_seq_len) {
        char buf[128];
        snprintf(buf, sizeof buf, "Input sequence length %d exceeds max_seq_len %d", pos0 + Lp, c.max_seq_len);
        return ft_fail(ctx, FT_ERR_TOO_LONG, buf);
    }
    const int R = c.num_codebooks + 1;
    ArTraceScope traced(ctx, true, 4, slot, 1);        // (inside a traced ft_ar_prefill_slow_many: that call's trace goes on)
    if (traced.own) tr_state(ctx, 0);
    ctx->hid_in_xo[slot] = 0;
    FT_TRY(ft_ar_reset(ctx, slot));
    FT_HIP(ctx, hipMemcpyAsync(ctx->d_prompt, prompt, (size_t)R * Lp * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    tr_uploaded(ctx, {TB_PROMPT});
    pick_nsplit(ctx, pos0 + Lp);
    Launch L{ctx, ctx->stream, slot, 1, 0};
    if (!ctx->prefill_v0) {
        prefill_gemm(L, slot, Lp, pos0, false);
    } else {
        for (int t = 0; t < Lp; ++t) {
            L.pos_off = pos0 + t;
            tr_pos(ctx, t);
            enqueue_slow_only(L, ctx->d_prompt, Lp, 0, t);
        }
    }
    if (L.err != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("prefill launch: ") + hipGetErrorString(L.err));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));   // d_prompt is reused by the next call
    if (traced.own) tr_state(ctx, 1);
    return FT_OK;
}

// Prompt passes of several slots (a batch scheduler's initial fill and its refills; per prompt: inference.py:353-362).
// Where lock-step batches run on the MFMA launches (ctx->wide_ok) and n reaches their width (wide_min), the prompts go
// through the slow stack TOGETHER: their positions back to back as the rows of one pass - every Linear product streams its
// weights once for all of them (a 48-position prompt alone is bound by the weight stream: 32 of them cost 32 streams) -
// while the K/V append goes by (slot, position) of each row and the attention by sequence (grid.z).  Like the lock-step
// frames of that width the products then sum in another order than a prompt pass on its own (another tile kernel from
// 129 rows): judged against the oracle with the bf16 margin.  Fewer prompts, other precisions (fp16 included) and shapes: one by one,
// bit-equal to ft_ar_prefill_slow.  More rows than the workspace holds (max_seq_len): several passes.
extern "C" ft_status ft_ar_prefill_slow_many(ft_ctx* ctx, int32_t n, const int32_t* slots, const int32_t* prompts,
                                             const int32_t* Lps, const int32_t* pos0s) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (!slots || !prompts || !Lps || !pos0s) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill_slow_many: null argument");
    if (n < 1 || n > c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill_slow_many: bad count");
    const int R = c.num_codebooks + 1;
    std::vector<char> seen(c.max_batch, 0);
    std::vector<size_t> off(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= c.max_batch || seen[slots[i]]) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill_slow_many: bad or repeated slot");
        seen[slots[i]] = 1;
        if (Lps[i] < 1 || pos0s[i] < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_prefill_slow_many: empty prompt");
        if (pos0s[i] + Lps[i] >= c.max_seq_len) {
            char buf[128];
            snprintf(buf, sizeof buf, "Input sequence length %d exceeds max_seq_len %d", pos0s[i] + Lps[i], c.max_seq_len);
            return ft_fail(ctx, FT_ERR_TOO_LONG, buf);
        }
        off[i + 1] = off[i] + (size_t)R * Lps[i];
    }
    // bf16 only (the pf_* workspace and the prompt kernels): fp16 runs its lock-step frames on the MFMA launches, its prompts one by one
    const bool ragged = c.dtype == FT_BF16 && !ctx->prefill_v0 && ctx->wide_ok && n >= ctx->wide_min && (c.head_dim == 64 || c.head_dim == 128) &&
                        !getenv("FT_PREFILL_ATTN_V0") && !getenv("FT_NO_RAGGED_PREFILL");
    ArTraceScope traced(ctx, true, 5, 0, n);           // one trace over every pass of the call, the single passes of the fall-back included
    if (traced.own) tr_state(ctx, 0);
    if (!ragged) {
        for (int i = 0; i < n; ++i) {
            if (traced.own && n > 1) ctx->tstore.pass_prefix = tr_name("pass%d.", i);
            FT_TRY(ft_ar_prefill_slow(ctx, slots[i], prompts + off[i], Lps[i], pos0s[i]));
        }
        if (traced.own) tr_state(ctx, 1);
        return FT_OK;
    }
    std::vector<int> tok;
    std::vector<int4> seqs;
    std::vector<int2> rows;
    for (int i0 = 0, pass = 0; i0 < n; ++pass) {
        int i1 = i0, S = 0, max_lp = 0, end = 0;
        while (i1 < n && S + Lps[i1] <= c.max_seq_len) { S += Lps[i1]; max_lp = std::max(max_lp, Lps[i1]); end = std::max(end, pos0s[i1] + Lps[i1]); ++i1; }
        if (traced.own && (pass > 0 || i1 < n)) ctx->tstore.pass_prefix = tr_name("pass%d.", pass);
        tok.assign((size_t)R * S, 0); seqs.clear(); rows.clear();
        int row0 = 0;
        for (int i = i0; i < i1; ++i) {
            ctx->hid_in_xo[slots[i]] = 0;       // as a single pass: the slot's hidden state is the row this pass leaves in ctx->x
            FT_TRY(ft_ar_reset(ctx, slots[i]));
            for (int r = 0; r < R; ++r)
                memcpy(&tok[(size_t)r * S + row0], prompts + off[i] + (size_t)r * Lps[i], (size_t)Lps[i] * sizeof(int));
            seqs.push_back(int4{row0, Lps[i], pos0s[i], slots[i]});
            for (int t = 0; t < Lps[i]; ++t) rows.push_back(int2{slots[i], pos0s[i] + t});
            row0 += Lps[i];
        }
        FT_HIP(ctx, hipMemcpyAsync(ctx->d_prompt, tok.data(), tok.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        FT_HIP(ctx, hipMemcpyAsync(ctx->pf_seqs, seqs.data(), seqs.size() * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
        FT_HIP(ctx, hipMemcpyAsync(ctx->pf_rows, rows.data(), rows.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
        tr_uploaded(ctx, {TB_PROMPT, TB_PF_SEQS, TB_PF_ROWS});
        pick_nsplit(ctx, end);
        Launch L{ctx, ctx->stream, 0, 1, 0};
        const RaggedPf rg{i1 - i0, max_lp};
        prefill_gemm(L, 0, S, 0, false, &rg);
        if (L.err != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("prefill launch: ") + hipGetErrorString(L.err));
        FT_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the host vectors and d_prompt are reused by the next pass
        i0 = i1;
    }
    if (traced.own) tr_state(ctx, 1);
    return FT_OK;
}

// First frames of slots [slot0, slot0 + n) whose prompts went through ft_ar_prefill_slow: one lock-step pass of the
// vocabulary head, the semantic draw and the fast codebooks over all of them.
extern "C" ft_status ft_ar_first_frames(ft_ctx* ctx, int32_t slot0, int32_t n, const ft_sampling* sp, const int32_t* next_pos,
                                        int32_t* out_frames) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (!sp || !next_pos || !out_frames) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_first_frames: null argument");
    if (slot0 < 0 || n < 1 || slot0 + n > c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_first_frames: bad slot range");
    const int R = c.num_codebooks + 1;
    const bool on_engine = n == 1 && eng_in_use(ctx);
    if (ctx->tstore.armed && on_engine) {
        ctx->tstore.armed = false;
        return ft_fail(ctx, FT_ERR_STATE, "ft_ar_first_frames: a traced call never runs on the frame engine");
    }
    ArTraceScope traced(ctx, true, 2, slot0, n);
    FT_TRY(upload_ctl(ctx, slot0, n, sp));
    if (ctx->trace) tr_state(ctx, 0);
    Launch L{ctx, ctx->stream, slot0, n, 0};
    L.tail_only = true;
    auto tail = [&]() -> ft_status {
        enqueue_tail(L);
        return L.err == hipSuccess ? FT_OK : ft_fail(ctx, FT_ERR_HIP, std::string("first-frame launch: ") + hipGetErrorString(L.err));
    };
    FT_TRY(tail());
    // as in ft_ar_prefill_at: a timed-out codebook loop is redone on the launch path
    if (on_engine) FT_TRY(eng_fallback(ctx, [&] { return ft_ar_reset(ctx, slot0); }, tail));
    // finalize() advanced every position 0 -> 1; the next input position of a slot is the end of its prompt
    FT_HIP(ctx, hipMemcpyAsync(ctx->d_pos + slot0, next_pos, n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FT_HIP(ctx, hipMemcpyAsync(out_frames, ctx->d_tok + (size_t)slot0 * R, (size_t)n * R * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int m = slot0; m < slot0 + n; ++m) ctx->hid_in_xo[m] = 0;    // a prompt pass leaves the rows' residual stream in ctx->x
    if (ctx->trace) tr_state(ctx, 1);
    return FT_OK;
}

extern "C" ft_status ft_ar_prefill(ft_ctx* ctx, int32_t slot, const int32_t* prompt, int32_t Lp,
                                   const ft_sampling* sp, int32_t* out_frame) {
    return ft_ar_prefill_at(ctx, slot, prompt, Lp, 0, sp, out_frame);
}

// ---- reference-prefix K/V snapshots: [layer][K|V][Hkv][n_pos][hd] packed, in the cache's element type
struct ft_kv_snapshot {
    char* data = nullptr;
    int n_pos = 0;
    size_t bytes = 0;
};

static ft_status kv_copy(ft_ctx* ctx, char* snap, int n_pos, int slot, bool save) {
    const ft_ar_config& c = ctx->c;
    const size_t row = (size_t)n_pos * c.head_dim * ctx->esz;            // one head's positions [0, n_pos)
    const size_t pitch = (size_t)ctx->n_slots * c.head_dim * ctx->esz;   // head stride inside the cache
    for (int li = 0; li < c.n_layer; ++li) {
        const FtLayer& l = ctx->layers[li];
        for (int kv = 0; kv < 2; ++kv) {
            char* cache = (char*)(kv ? l.vc : l.kc) + (size_t)slot * ctx->cache_m_stride * ctx->esz;
            char* packed = snap + ((size_t)li * 2 + kv) * c.n_local_heads * row;
            if (save) FT_HIP(ctx, hipMemcpy2DAsync(packed, row, cache, pitch, row, c.n_local_heads, hipMemcpyDeviceToDevice, ctx->stream));
            else FT_HIP(ctx, hipMemcpy2DAsync(cache, pitch, packed, row, row, c.n_local_heads, hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    return FT_OK;
}

extern "C" ft_status ft_ar_kv_save(ft_ctx* ctx, int32_t slot, int32_t n_pos, ft_kv_snapshot** out) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (!out) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_kv_save: null argument");
    if (slot < 0 || slot >= c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_kv_save: bad slot");
    if (n_pos < 1 || n_pos > ctx->n_slots) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_kv_save: bad n_pos");
    ft_kv_snapshot* s = new ft_kv_snapshot();
    s->n_pos = n_pos;
    s->bytes = (size_t)c.n_layer * 2 * c.n_local_heads * n_pos * c.head_dim * ctx->esz;
    if (hipMalloc((void**)&s->data, s->bytes) != hipSuccess) {
        delete s;
        return ft_fail(ctx, FT_ERR_HIP, "ft_ar_kv_save: out of device memory");
    }
    ft_status st = kv_copy(ctx, s->data, n_pos, slot, true);
    if (st == FT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = ft_fail(ctx, FT_ERR_HIP, "ft_ar_kv_save: copy failed");
    if (st != FT_OK) { hipFree(s->data); delete s; return st; }
    *out = s;
    return FT_OK;
}

extern "C" ft_status ft_ar_kv_restore(ft_ctx* ctx, const ft_kv_snapshot* snap, int32_t slot) {
    FT_TRY(ar_ready(ctx));
    if (!snap || !snap->data) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_kv_restore: null snapshot");
    if (slot < 0 || slot >= ctx->c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_kv_restore: bad slot");
    if (snap->n_pos > ctx->n_slots) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_kv_restore: snapshot longer than the cache");
    return kv_copy(ctx, snap->data, snap->n_pos, slot, false);  // stream-ordered before the next prefill
}

extern "C" int32_t ft_ar_kv_positions(const ft_kv_snapshot* snap) { return snap ? snap->n_pos : 0; }

extern "C" void ft_ar_kv_free(ft_ctx* ctx, ft_kv_snapshot* snap) {
    if (!snap) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    if (snap->data) hipFree(snap->data);
    delete snap;
}

// the captured grids depend on the batch width, on the KV split count and on whether the frame engine serves the frame
static int graph_key(const ft_ctx* ctx, int M, int frames) {
    const bool eng = M == 1 && (ctx->eng_on || ctx->eng_fast_on) && !ctx->eng_suspended;   // the engine serves one-slot frames only
    return (M * 64 + ctx->nsplit) + (frames > 1 ? frames * (1 << 20) : 0) + (eng ? (1 << 28) : 0);
}

static ft_status get_graph(ft_ctx* ctx, int M, hipGraphExec_t* out, int frames = 1) {
    // the captured grids depend on the batch width and on the KV split count; `frames` decode frames per graph
    const int key = graph_key(ctx, M, frames);
    auto it = ctx->graphs.find(key);
    if (it != ctx->graphs.end()) { *out = it->second; return FT_OK; }
    const int R = ctx->c.num_codebooks + 1;
    hipGraph_t graph = nullptr;
    FT_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    Launch L{ctx, ctx->stream, 0, M, 0};
    for (int f = 0; f < frames; ++f) enqueue_frame(L, ctx->d_tok, 1, R, 0);
    hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
    if (L.err != hipSuccess) e = L.err;
    if (e != hipSuccess) {
        if (graph) hipGraphDestroy(graph);
        return ft_fail(ctx, FT_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e));
    }
    hipGraphExec_t exec = nullptr;
    { size_t nn = 0; if (frames == 1 && hipGraphGetNodes(graph, nullptr, &nn) == hipSuccess) ctx->graph_nodes[key] = (int)nn; }
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(e));
    ctx->graphs[key] = exec;
    *out = exec;
    return FT_OK;
}

extern "C" ft_status ft_ar_decode(ft_ctx* ctx, int32_t nslots, int32_t n_frames, const ft_sampling* sp,
                                  int32_t poll, int32_t* out_frames, int32_t* out_n) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (!sp || !out_frames || !out_n) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_decode: null argument");
    if (nslots < 1 || nslots > c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_decode: bad nslots");
    if (n_frames < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_decode: n_frames < 0");
    if (poll < 1) poll = 1;
    const int R = c.num_codebooks + 1;
    if (ctx->tstore.armed && n_frames == 1 && nslots == 1 && eng_in_use(ctx)) {
        ctx->tstore.armed = false;
        return ft_fail(ctx, FT_ERR_STATE, "ft_ar_decode: a traced call never runs on the frame engine");
    }
    ArTraceScope traced(ctx, n_frames == 1, 1, 0, nslots);
    FT_TRY(upload_ctl(ctx, 0, nslots, sp));
    // state at entry
    int* h = ctx->h_pin;
    FT_HIP(ctx, hipMemcpyAsync(h, ctx->d_nf, nslots * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FT_HIP(ctx, hipMemcpyAsync(h + nslots, ctx->d_pos, nslots * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FT_HIP(ctx, hipMemcpyAsync(h + 2 * nslots, ctx->d_done, nslots * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> nf0(h, h + nslots);
    int budget = n_frames;
    for (int m = 0; m < nslots; ++m) {
        if (nf0[m] < 1) return ft_fail(ctx, FT_ERR_STATE, "ft_ar_decode: slot has not been prefilled");
        if (h[2 * nslots + m]) continue;  // finished or parked: frozen on the device, limits nothing
        budget = std::min(budget, ctx->cap - nf0[m]);
        // cache positions left: the rope table has max_seq_len rows (the cache's n_slots is that rounded up to 8)
        budget = std::min(budget, c.max_seq_len - h[nslots + m]);
    }
    if (budget < 0) budget = 0;
    // A row that drew <|im_end|> at its last cache row is frozen at position max_seq_len, and the attention launches take no
    // done flag: while the caller keeps it in the lock-step batch they would append at that row (the next kv head's, the next
    // slot's or nobody's) and read the rope table past its end.  Its position goes back inside its own cache: the row it
    // rewrites there is one no frame reads again.
    for (int m = 0; m < nslots; ++m)
        if (h[2 * nslots + m] && h[nslots + m] >= c.max_seq_len) {
            h[nslots + m] = c.max_seq_len - 1;
            FT_HIP(ctx, hipMemcpyAsync(ctx->d_pos + m, h + nslots + m, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        }
    if (ctx->trace) tr_state(ctx, 0);
    {   // KV splits follow the longest context this call will reach
        int pos_end = 0;
        for (int m = 0; m < nslots; ++m)
            if (!h[2 * nslots + m]) pos_end = std::max(pos_end, h[nslots + m] + budget);
        pick_nsplit(ctx, pos_end);
    }
    const bool eager = getenv("FT_NO_GRAPH") != nullptr || ctx->trace;   // a traced frame is launched, never captured or replayed
    // several frames per graph launch where a burst allows: the gap between two graph launches is ~7 us (measured: 687 ->
    // 692 tok/s at 16 frames per graph; the frames are the same launches in the same order)
    constexpr int gk = 16;
    const int first_burst = std::min(poll, budget);
    // `burst` frames on the stream, then the done flags: graph replays (16 / 4 / 1 frames per launch) or eager launches
    auto run_burst = [&](int burst) -> ft_status {
        hipGraphExec_t exec = nullptr, exec_k = nullptr, exec_4 = nullptr;
        if (!eager) FT_TRY(get_graph(ctx, nslots, &exec));
        if (!eager && gk > 1 && first_burst >= gk && burst >= gk) FT_TRY(get_graph(ctx, nslots, &exec_k, gk));
        if (!eager && gk > 4 && first_burst >= 4 && burst >= 4) FT_TRY(get_graph(ctx, nslots, &exec_4, 4));
        int i0 = 0;
        if (exec_k) for (; i0 + gk <= burst; i0 += gk) FT_HIP(ctx, hipGraphLaunch(exec_k, ctx->stream));
        if (exec_4) for (; i0 + 4 <= burst; i0 += 4) FT_HIP(ctx, hipGraphLaunch(exec_4, ctx->stream));
        for (int i = i0; i < burst; ++i) {
            if (eager) {
                Launch L{ctx, ctx->stream, 0, nslots, 0};
                enqueue_frame(L, ctx->d_tok, 1, R, 0);
                if (L.err != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("frame launch: ") + hipGetErrorString(L.err));
            } else {
                FT_HIP(ctx, hipGraphLaunch(exec, ctx->stream));
            }
        }
        FT_HIP(ctx, hipMemcpyAsync(h, ctx->d_done, nslots * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FT_OK;
    };
    const int pos0 = h[nslots], done0 = h[2 * nslots];      // slot 0 at entry (the engine serves one-slot calls only)
    std::vector<char> was_done(nslots);
    for (int m = 0; m < nslots; ++m) was_done[m] = (char)(h[2 * nslots + m] != 0);   // frozen slots produce nothing new
    int done_frames = 0;
    while (done_frames < budget) {
        const int burst = std::min(poll, budget - done_frames);
        const bool on_engine = nslots == 1 && eng_in_use(ctx);
        FT_TRY(run_burst(burst));
        if (on_engine) {
            FT_TRY(eng_fallback(ctx, [&]() -> ft_status {
                // slot 0 back to where this burst began (its frames [nf0 + done_frames, ..) and cache rows are rewritten by
                // the redo; the draws are counter-based, so the redo draws what the engine would have drawn), then the same
                // frames on the launch path
                int* hp = ctx->h_pin + 3 * nslots;
                hp[0] = done0 ? pos0 : pos0 + done_frames; hp[1] = done0 ? nf0[0] : nf0[0] + done_frames; hp[2] = done0;
                FT_HIP(ctx, hipMemcpyAsync(ctx->d_pos, hp, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
                FT_HIP(ctx, hipMemcpyAsync(ctx->d_nf, hp + 1, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
                FT_HIP(ctx, hipMemcpyAsync(ctx->d_done, hp + 2, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
                FT_HIP(ctx, hipMemcpy2DAsync(ctx->d_tok, sizeof(int), ctx->d_seq + (hp[1] - 1), (size_t)ctx->cap * sizeof(int),
                                             sizeof(int), R, hipMemcpyDeviceToDevice, ctx->stream));
                // the frame store beyond the rewound frame count goes back to zero: early in an utterance the repetition
                // penalty's window reaches past the current frame (inference.py:187-191 reads a 16-column window of a
                // zero-initialised store), and the aborted burst left its frames there
                if (!done0 && hp[1] < ctx->cap)
                    FT_HIP(ctx, hipMemset2DAsync(ctx->d_seq + hp[1], (size_t)ctx->cap * sizeof(int), 0,
                                                 (size_t)std::min(burst, ctx->cap - hp[1]) * sizeof(int), R, ctx->stream));
                return FT_OK;
            }, [&] { return run_burst(burst); }));
        }
        done_frames += burst;
        bool all = true;
        for (int m = 0; m < nslots; ++m) all = all && h[m];
        if (all) break;
    }
    // collect: frames [nf0, nf0+done_frames) of each slot, cut after the first <|im_end|>.  Only the columns
    // [nf0-1, nf0+done_frames) of the frame store travel (one strided copy per slot, all issued before the wait).
    const int W = done_frames + 1;
    std::vector<int> seq((size_t)nslots * R * W);
    for (int m = 0; m < nslots; ++m) {
        if (was_done[m] || done_frames == 0) continue;
        const int c0 = std::min(nf0[m] - 1, ctx->cap - W);        // stay inside the store near its end
        FT_HIP(ctx, hipMemcpy2DAsync(seq.data() + (size_t)m * R * W, (size_t)W * sizeof(int),
                                     ctx->d_seq + (size_t)m * R * ctx->cap + std::max(c0, 0), (size_t)ctx->cap * sizeof(int),
                                     (size_t)std::min(W, ctx->cap) * sizeof(int), R, hipMemcpyDeviceToHost, ctx->stream));
    }
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int m = 0; m < nslots; ++m) {
        int n = 0;
        if (!was_done[m] && done_frames > 0) {
            const int c0 = std::max(std::min(nf0[m] - 1, ctx->cap - W), 0);
            const int* sm = seq.data() + (size_t)m * R * W;
            for (int f = 0; f < done_frames; ++f) {
                const int col = nf0[m] + f - c0;
                if (col >= std::min(W, ctx->cap)) break;
                for (int r = 0; r < R; ++r) out_frames[((size_t)m * n_frames + f) * R + r] = sm[(size_t)r * W + col];
                n = f + 1;
                if (sm[col] == c.im_end_id) break;
            }
        }
        out_n[m] = n;
    }
    if (done_frames > 0) {   // ft_ar_get_debug: where these rows' residual stream is
        Launch L{ctx, ctx->stream, 0, nslots, 0};
        for (int m = 0; m < nslots; ++m) ctx->hid_in_xo[m] = wide_batch(L) ? 1 : 0;
    }
    if (ctx->trace) tr_state(ctx, 1);
    return FT_OK;
}

// A hand-off time-out of the frame engine (ENG_CTL_ABORT: some workgroup gave up after ENG_TIMEOUT_TICKS, then all did)
// is survivable.  Called after the stream has drained: *aborted tells the caller that the frames since the last check
// are invalid; the control words and every hand-off buffer are cleared (no granule of the aborted launches can carry a
// valid tag afterwards: tag 0 is never valid and the epoch moves on), and after ENG_MAX_STRIKES events the context stops
// using the engine.  The caller then redoes those frames on the launch path (ctx->eng_suspended).
static ft_status eng_recover(ft_ctx* ctx, bool* aborted) {
    *aborted = false;
    if (!ctx->eng_ctl) return FT_OK;
    unsigned w[ENG_CTL_WORDS];
    FT_HIP(ctx, hipMemcpyAsync(w, ctx->eng_ctl, sizeof w, hipMemcpyDeviceToHost, ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!w[ENG_CTL_ABORT]) return FT_OK;
    *aborted = true;
    ctx->eng_strikes += 1;
    ctx->eng_last_where = (int)w[ENG_CTL_WHERE];
    const unsigned epoch = w[ENG_CTL_EPOCH] + 4u * ENG_EPOCH_STEP;
    FT_HIP(ctx, hipMemsetAsync(ctx->eng_ctl, 0, ENG_CTL_WORDS * 4, ctx->stream));
    FT_HIP(ctx, hipMemcpyAsync(ctx->eng_ctl + ENG_CTL_EPOCH, &epoch, sizeof epoch, hipMemcpyHostToDevice, ctx->stream));
    if (ctx->eng_gx) FT_HIP(ctx, hipMemsetAsync(ctx->eng_gx, 0, ctx->eng_pool_bytes, ctx->stream));
    if (ctx->eng_gpart) FT_HIP(ctx, hipMemsetAsync(ctx->eng_gpart, 0, ctx->eng_gpart_bytes, ctx->stream));
    if (ctx->eng_fast_g) FT_HIP(ctx, hipMemsetAsync(ctx->eng_fast_g, 0, ctx->eng_fast_bytes, ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (epoch is a stack word)
    char buf[256];
    if (ctx->eng_strikes >= ENG_MAX_STRIKES) {
        // the engine is given up for good: its graphs go, its buffers and the device's engine seat are released (another
        // context of the process may take it), the reason stays readable through ft_ar_frame_path
        for (auto it = ctx->graphs.begin(); it != ctx->graphs.end();) {
            if (it->first & (1 << 28)) { hipGraphExecDestroy(it->second); it = ctx->graphs.erase(it); } else ++it;
        }
        eng_release(ctx);
        snprintf(buf, sizeof buf, "launch path: the frame engine was turned off after %d hand-off time-outs (last in phase %u)",
                 ctx->eng_strikes, w[ENG_CTL_WHERE]);
        ctx->eng_why = buf;
    }
    fprintf(stderr, "fish_tts_amd: frame engine: a hand-off timed out (phase %u, strike %d of %d): the frames are redone on the "
            "launch path%s\n", w[ENG_CTL_WHERE], ctx->eng_strikes, ENG_MAX_STRIKES,
            ctx->eng_strikes >= ENG_MAX_STRIKES ? "; the engine stays off for this context" : "");
    return FT_OK;
}
static bool eng_in_use(const ft_ctx* ctx) { return (ctx->eng_on || ctx->eng_fast_on) && !ctx->eng_suspended; }

extern "C" ft_status ft_ar_engine_state(ft_ctx* ctx, int32_t* flags, int32_t* aborted, int32_t* where) {
    FT_TRY(ar_ready(ctx));
    if (flags) *flags = (ctx->eng_on ? 1 : 0) | (ctx->eng_fast_on ? 2 : 0);
    if (aborted) *aborted = ctx->eng_strikes;
    if (where) *where = ctx->eng_last_where;
    return FT_OK;
}

extern "C" const char* ft_ar_frame_path(const ft_ctx* ctx) {
    if (!ctx) return "";
    // batch-1 frames, then what a lock-step batch of >= wide_min rows runs on
    ft_ctx* c = const_cast<ft_ctx*>(ctx);
    c->path_str = ctx->eng_why + (ctx->wide_ok
                                      ? "; lock-step batches of >= 5 rows: MFMA launches with fused row operations (five per layer)"
                                      : "; lock-step batches: multi-row GEMV launches");
    return c->path_str.c_str();
}

// Test hook: workgroup `wg` of a coming slow-stack (which = 0) or codebook-loop (which = 1) engine launch plays dead - it
// publishes nothing, every workgroup that waits for its rows times out (one shot: that workgroup clears the word).  `skip`
// launches of that kind pass first, so the time-out can be placed in a later burst of a call or inside a multi-frame graph.
extern "C" ft_status ft_test_engine_fault(ft_ctx* ctx, int32_t which, int32_t wg, int32_t skip) {
    FT_TRY(ar_ready(ctx));
    if (!ctx->eng_ctl || !(which == 0 ? ctx->eng_on : ctx->eng_fast_on)) return ft_fail(ctx, FT_ERR_STATE, "ft_test_engine_fault: the frame engine is off");
    if (wg < 0 || wg >= ctx->eng_nb || skip < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_engine_fault: bad workgroup or skip count");
    const unsigned v[2] = {(which == 0 ? 0u : ENG_FAULT_FAST) + 1u + (unsigned)wg, (unsigned)skip};
    static_assert(ENG_CTL_FAULT_SKIP == ENG_CTL_FAULT + 1, "the two words are written by one copy");
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FT_HIP(ctx, hipMemcpy(ctx->eng_ctl + ENG_CTL_FAULT, v, sizeof v, hipMemcpyHostToDevice));
    return FT_OK;
}

// Test hook: what the attention of the last prefill / decode call ran on: its KV split count (pick_nsplit), whether the
// slow-stack engine of this context is the XCD-local kernel, and the rows of the cache.  Host fields only.
extern "C" ft_status ft_test_ar_attn_plan(ft_ctx* ctx, int32_t* nsplit, int32_t* xl, int32_t* n_slots) {
    FT_TRY(ar_ready(ctx));
    if (nsplit) *nsplit = ctx->nsplit;
    if (xl) *xl = ctx->eng_on && ctx->eng_xl ? 1 : 0;
    if (n_slots) *n_slots = ctx->n_slots;
    return FT_OK;
}

// Test hook: the per-slot state of every slot, whole (include/fishtts_hip_test.h).  Host code: the stream is drained, then
// one copy per array (and per layer's K and V cache) to the host.
extern "C" ft_status ft_test_ar_slots(ft_ctx* ctx, int32_t* geo, int32_t* tok, int32_t* tokn, int32_t* pos, int32_t* nf, int32_t* done,
                                      int32_t* seq, uint32_t* ctl, uint8_t* hid_in_xo, void* kv) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    const size_t MB = c.max_batch, R = c.num_codebooks + 1, W = sizeof(RowCtl) / sizeof(uint32_t);
    static_assert(sizeof(RowCtl) % sizeof(uint32_t) == 0, "the sampling rows are read as whole words");
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (geo) {
        const int32_t g[10] = {c.max_batch, (int32_t)R, ctx->cap, (int32_t)W, c.n_layer, c.n_local_heads, ctx->n_slots, c.head_dim,
                               (int32_t)ctx->esz, c.im_end_id};
        memcpy(geo, g, sizeof g);
    }
    auto out = [&](void* dst, const void* src, size_t bytes) { return dst ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
    FT_HIP(ctx, out(tok, ctx->d_tok, MB * R * 4));
    FT_HIP(ctx, out(tokn, ctx->d_tokn, MB * R * 4));
    FT_HIP(ctx, out(pos, ctx->d_pos, MB * 4));
    FT_HIP(ctx, out(nf, ctx->d_nf, MB * 4));
    FT_HIP(ctx, out(done, ctx->d_done, MB * 4));
    FT_HIP(ctx, out(seq, ctx->d_seq, MB * R * ctx->cap * 4));
    FT_HIP(ctx, out(ctl, ctx->d_ctl, MB * sizeof(RowCtl)));
    if (hid_in_xo) for (size_t m = 0; m < MB; ++m) hid_in_xo[m] = ctx->hid_in_xo[m] ? 1 : 0;
    if (kv) {
        const size_t bytes = MB * ctx->cache_m_stride * ctx->esz;            // one layer's K or V cache, every slot
        for (int li = 0; li < c.n_layer; ++li) {
            FT_HIP(ctx, hipMemcpy((char*)kv + ((size_t)li * 2) * bytes, ctx->layers[li].kc, bytes, hipMemcpyDeviceToHost));
            FT_HIP(ctx, hipMemcpy((char*)kv + ((size_t)li * 2 + 1) * bytes, ctx->layers[li].vc, bytes, hipMemcpyDeviceToHost));
        }
    }
    return FT_OK;
}

// Test hook: the hand-off vectors the engine's launches left behind, and K/V rows (include/fishtts_hip_test.h).  Host code:
// one copy of each pool to the host, then the decoding below with the layout rules of frame_engine.h.
namespace {
// ---- launch trace hooks of the AR frame (fishtts_hip_test.h)
extern "C" ft_status ft_test_ar_trace_arm(ft_ctx* ctx, int32_t first, int32_t count) {
    FT_TRY(ar_ready(ctx));
    if (first < 0 || count < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_ar_trace_arm: bad range");
    if (ctx->c.max_batch == 1 && eng_in_use(ctx))
        return ft_fail(ctx, FT_ERR_STATE, "ft_test_ar_trace_arm: this context's frames run on the frame engine");
    ArTrace& t = ctx->tstore;
    t.recs.clear();
    t.first = first; t.count = count; t.armed = true; t.failed = false; t.kind = 0;
    return FT_OK;
}
extern "C" int32_t ft_test_ar_trace_count(ft_ctx* ctx, int32_t* info) {
    if (!ctx || !ctx->has_ar) return -1;
    const ArTrace& t = ctx->tstore;
    if (info) { info[0] = t.kind; info[1] = t.m0; info[2] = t.M; info[3] = t.armed ? 1 : 0; info[4] = (int32_t)t.begin.size(); }
    return t.failed ? -1 : (int32_t)t.recs.size();
}
extern "C" ft_status ft_test_ar_trace_launch(ft_ctx* ctx, int32_t i, char* name, int32_t cap, int32_t* info) {
    if (!ctx || !ctx->has_ar || !name || cap < 1 || !info) return FT_ERR_ARG;
    const ArTrace& t = ctx->tstore;
    if (i < 0 || i >= (int)t.recs.size()) return ft_fail(ctx, FT_ERR_ARG, "ft_test_ar_trace_launch: no such launch");
    const ArTraceRec& r = t.recs[i];
    snprintf(name, (size_t)cap, "%s", r.name.c_str());
    info[0] = r.m0; info[1] = r.rows; info[2] = r.cols; info[3] = (int32_t)r.bufs.size(); info[4] = r.held ? 1 : 0;
    for (int k = 0; k < 4; ++k) info[5 + k] = r.cls[k];
    info[9] = r.pos_off;
    return FT_OK;
}
extern "C" ft_status ft_test_ar_trace_buffer(ft_ctx* ctx, int32_t i, int32_t j, int32_t* info, void* dst) {
    if (!ctx || !ctx->has_ar || !info) return FT_ERR_ARG;
    ArTrace& t = ctx->tstore;
    std::vector<ArTraceBuf>* bufs = i == -1 ? &t.begin : i >= 0 && i < (int)t.recs.size() ? &t.recs[i].bufs : nullptr;
    if (!bufs || j < 0 || j >= (int)bufs->size()) return ft_fail(ctx, FT_ERR_ARG, "ft_test_ar_trace_buffer: no such buffer");
    ArTraceBuf& b = (*bufs)[j];
    info[0] = b.id; info[1] = b.esz; info[2] = b.rows; info[3] = b.cols;
    if (dst) {
        if (b.data.empty()) return ft_fail(ctx, FT_ERR_STATE, "ft_test_ar_trace_buffer: launch outside the armed range, or read before");
        memcpy(dst, b.data.data(), b.data.size());
        std::vector<char>().swap(b.data);   // handed over
    }
    return FT_OK;
}
extern "C" ft_status ft_test_ar_trace_state(ft_ctx* ctx, int32_t which, int32_t* tok, int32_t* pos, int32_t* nf, int32_t* done, int32_t* seq) {
    if (!ctx || !ctx->has_ar || (which != 0 && which != 1) || !tok || !pos || !nf || !done || !seq) return FT_ERR_ARG;
    const ArTraceState& s = ctx->tstore.st[which];
    if (ctx->tstore.kind == 0 || s.pos.empty()) return ft_fail(ctx, FT_ERR_STATE, "ft_test_ar_trace_state: no traced call");
    memcpy(tok, s.tok.data(), s.tok.size() * 4); memcpy(pos, s.pos.data(), s.pos.size() * 4); memcpy(nf, s.nf.data(), s.nf.size() * 4);
    memcpy(done, s.done.data(), s.done.size() * 4); memcpy(seq, s.seq.data(), s.seq.size() * 4);
    return FT_OK;
}

struct EngDump {
    const unsigned* w;      // one copy of a pool on the host
    // n plain granules {tag16 | bf16} of a vector stored linearly (EngLayout::off is the identity) from word `at`
    void plain(size_t at, int n, uint16_t* v, uint16_t* t) const {
        for (int i = 0; i < n; ++i) { v[i] = (uint16_t)(w[at + i] & 0xffffu); t[i] = (uint16_t)(w[at + i] >> 16); }
    }
    // n values as PK3 granules {v0 | v1 << 16, v2 | tag << 16}: granule j holds values 3 j .. 3 j + 2 under one tag
    void pk3(size_t at, int n, uint16_t* v, uint16_t* t) const {
        for (int j = 0; j < n / 3; ++j) {
            const unsigned w0 = w[at + 2 * j], w1 = w[at + 2 * j + 1];
            v[3 * j] = (uint16_t)(w0 & 0xffffu); v[3 * j + 1] = (uint16_t)(w0 >> 16); v[3 * j + 2] = (uint16_t)(w1 & 0xffffu);
            t[3 * j] = t[3 * j + 1] = t[3 * j + 2] = (uint16_t)(w1 >> 16);
        }
    }
};
}  // namespace

extern "C" ft_status ft_test_engine_handoffs(ft_ctx* ctx, ft_test_engine_io* io) {
    FT_TRY(ar_ready(ctx));
    if (!io || (io->which != 0 && io->which != 1)) return ft_fail(ctx, FT_ERR_ARG, "ft_test_engine_handoffs: bad argument");
    const ft_ar_config& c = ctx->c;
    const bool fast = io->which == 1;
    const bool on = fast ? ctx->eng_fast_on : ctx->eng_on;
    const int room = io->copies;
    const int nL = fast ? c.n_fast_layer : c.n_layer;
    const int H = fast ? c.fast_n_head : c.n_head, Hkv = fast ? c.fast_n_local_heads : c.n_local_heads;
    const int hd = fast ? c.fast_head_dim : c.head_dim;
    const int D = fast ? c.fast_dim : c.dim, F = fast ? c.fast_intermediate_size : c.intermediate_size;
    const int HD = H * hd, QKVN = (H + 2 * Hkv) * hd, V = fast ? ctx->fastV : 0;
    const int nb = ctx->eng_nb;
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    io->copies = on ? (ctx->eng_relay ? 9 : 1) : 0;
    io->epoch = 0; io->epoch_step = ENG_EPOCH_STEP; io->line = ENG_LINE;
    io->n_layer = nL; io->D = D; io->QKVN = QKVN; io->HD = HD; io->F = F; io->V = V; io->ncb = c.num_codebooks;
    io->H = H; io->Hkv = Hkv; io->hd = hd;
    io->pk3 = on && F % 384 == 0 && nb > 0 && (F / nb) % 3 == 0 ? 1 : 0;      // EngSlowShape / EngFastShape::PK3
    io->pair = fast && on && ctx->eng_pair && c.num_codebooks >= 2 ? 1 : 0;
    io->qkv0 = fast && on && ctx->eng_qkv0_tab ? 1 : 0;
    io->resident = 0;
    if (fast && on) {
        int n = 0;
        const EngFastEntry* tab = eng_fast_shapes(&n);
        for (int i = 0; i < n; ++i) if (tab[i].resident && (const void*)tab[i].resident == ctx->eng_fast_fn) io->resident = 1;
    }
    io->relay = on && ctx->eng_relay ? 1 : 0;
    io->xl = !fast && on && ctx->eng_xl ? 1 : 0;
    io->nsplit = fast ? 1 : ctx->nsplit;
    if (on) FT_HIP(ctx, hipMemcpy(&io->epoch, ctx->eng_ctl + ENG_CTL_EPOCH, sizeof(unsigned), hipMemcpyDeviceToHost));
    const bool want = io->x || io->qkv || io->xb || io->g || io->g3 || io->log || io->y || io->code || io->part;
    if (want && !on) return ft_fail(ctx, FT_ERR_STATE, "ft_test_engine_handoffs: that engine is off on this context");
    if (want && room < io->copies) return ft_fail(ctx, FT_ERR_STATE, "ft_test_engine_handoffs: room for fewer copies than exist");
    if (want && ((io->x && !io->x_tag) || (io->qkv && !io->qkv_tag) || (io->xb && !io->xb_tag) || (io->g && !io->g_tag) ||
                 (io->g3 && !io->g3_tag) || (io->log && !io->log_tag) || (io->y && !io->y_tag) || (io->part && !io->part_tag)))
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_engine_handoffs: a value array without its tag array");
    if (want) {
        const size_t VW = (size_t)nb * ENG_LINE;                      // words per vector buffer (the kernels' VSTR)
        const size_t words = fast ? ctx->eng_fast_words : ctx->eng_pool_words;
        const unsigned* dev = fast ? ctx->eng_fast_g : ctx->eng_gx;
        std::vector<unsigned> host(words);
        const size_t L = (size_t)nL;
        // word offsets of the vectors inside one copy of the pool, as the launches lay them out
        // (enqueue_fast_engine: gx gqkv gxb gg glog gcode; eng_setup_try: gx gxb gg gy gqkv)
        const size_t f_gx = 0, f_gq = 2 * (L + 1) * VW, f_gxb = f_gq + 2 * L * VW, f_gg = f_gxb + 2 * L * VW, f_log = f_gg + 2 * L * VW,
                     f_code = f_log + 2 * VW;
        const size_t s_gx = 0, s_gxb = (L + 1) * VW, s_gg = s_gxb + L * VW, s_gy = s_gg + L * VW, s_gq = s_gy + L * (size_t)HD;
        const int ns = io->nsplit > 0 ? io->nsplit : 1, G = H / Hkv, epb = hd / ns;
        for (int cp = 0; cp < io->copies; ++cp) {
            FT_HIP(ctx, hipMemcpy(host.data(), dev + (size_t)cp * words, words * sizeof(unsigned), hipMemcpyDeviceToHost));
            const EngDump d{host.data()};
            for (int par = 0; par < 2; ++par) {
                if (fast) {
                    for (int l = 0; l <= nL; ++l) {
                        const size_t o = ((size_t)cp * 2 + par) * (L + 1) + l;
                        if (io->x) d.plain(f_gx + ((size_t)par * (L + 1) + l) * VW, D, io->x + o * D, io->x_tag + o * D);
                        if (l == nL) continue;
                        const size_t q = ((size_t)cp * 2 + par) * L + l, b = ((size_t)par * L + l) * VW;
                        if (io->qkv) d.plain(f_gq + b, QKVN, io->qkv + q * QKVN, io->qkv_tag + q * QKVN);
                        if (io->xb) d.plain(f_gxb + b, D, io->xb + q * D, io->xb_tag + q * D);
                        if (io->g) d.plain(f_gg + b, F, io->g + q * F, io->g_tag + q * F);
                        if (io->g3 && io->pk3) d.pk3(f_gg + b, F, io->g3 + q * F, io->g3_tag + q * F);
                    }
                    const size_t o = (size_t)cp * 2 + par;
                    if (io->log) d.plain(f_log + (size_t)par * VW, V, io->log + o * V, io->log_tag + o * V);
                } else {
                    const size_t o = (size_t)cp * 2 + par;
                    const bool have = par < nL;                           // gqkv, gxb, gg, gy hold n_layer buffers, gx one more
                    auto zero = [&](uint16_t* v, uint16_t* t, size_t n) { if (v) { memset(v + o * n, 0, n * 2); memset(t + o * n, 0, n * 2); } };
                    if (io->x) d.plain(s_gx + (size_t)par * VW, D, io->x + o * D, io->x_tag + o * D);
                    if (!have) {
                        zero(io->qkv, io->qkv_tag, QKVN); zero(io->xb, io->xb_tag, D); zero(io->g, io->g_tag, F);
                        zero(io->g3, io->g3_tag, F); zero(io->y, io->y_tag, HD);
                        continue;
                    }
                    if (io->qkv) d.plain(s_gq + (size_t)par * VW, QKVN, io->qkv + o * QKVN, io->qkv_tag + o * QKVN);
                    if (io->xb) d.plain(s_gxb + (size_t)par * VW, D, io->xb + o * D, io->xb_tag + o * D);
                    if (io->g) d.plain(s_gg + (size_t)par * VW, F, io->g + o * F, io->g_tag + o * F);
                    if (io->g3 && io->pk3) d.pk3(s_gg + (size_t)par * VW, F, io->g3 + o * F, io->g3_tag + o * F);
                    if (io->y) {
                        // y is stored per attention workgroup, [kvh][split][g][hd / nsplit] (slow_engine_kernel: ymap)
                        for (int i = 0; i < HD; ++i) {
                            const int a2 = i / (G * epb), r2 = i % (G * epb), g2 = r2 / epb, eo = r2 % epb;
                            const int u = ((a2 / ns) * G + g2) * hd + (a2 % ns) * epb + eo;
                            const unsigned wv = host[s_gy + (size_t)par * HD + i];
                            io->y[o * HD + u] = (uint16_t)(wv & 0xffffu); io->y_tag[o * HD + u] = (uint16_t)(wv >> 16);
                        }
                    }
                }
            }
            if (fast && io->code)
                memcpy(io->code + (size_t)cp * c.num_codebooks * ENG_LINE, host.data() + f_code, (size_t)c.num_codebooks * ENG_LINE * sizeof(unsigned));
        }
        if (!fast && io->part) {
            const size_t per = (size_t)H * ns * (hd + 2);
            const int pars = nL < 2 ? nL : 2;
            std::vector<unsigned long long> hp(per * pars);
            FT_HIP(ctx, hipMemcpy(hp.data(), ctx->eng_gpart, hp.size() * 8, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < 2 * per; ++i) {
                const unsigned long long g = i < hp.size() ? hp[i] : 0ull;
                const unsigned lo = (unsigned)(g & 0xffffffffull);
                memcpy(io->part + i, &lo, 4);
                io->part_tag[i] = (unsigned)(g >> 32);
            }
        }
    }
    if (io->tab) {
        if (!fast || !on || !ctx->eng_qkv0_tab) return ft_fail(ctx, FT_ERR_STATE, "ft_test_engine_handoffs: this context built no layer-0 q k v table for the loop");
        if (io->tab_row < 0 || io->tab_row >= ctx->fastV) return ft_fail(ctx, FT_ERR_ARG, "ft_test_engine_handoffs: bad table row");
        FT_HIP(ctx, hipMemcpy(io->tab, (const bf16_t*)ctx->eng_qkv0_tab + (size_t)io->tab_row * QKVN, (size_t)QKVN * sizeof(bf16_t), hipMemcpyDeviceToHost));
    }
    if (io->kv_k || io->kv_v) {
        if (!io->kv_k || !io->kv_v) return ft_fail(ctx, FT_ERR_ARG, "ft_test_engine_handoffs: K/V needs both arrays");
        const size_t esz = ctx->esz;      // an f32 context: the arrays hold f32 values (twice the room)
        const int rows_max = fast ? c.num_codebooks : ctx->n_slots;
        if (io->kv_layer < 0 || io->kv_layer >= nL || io->kv_slot < 0 || io->kv_slot >= c.max_batch || io->kv_rows < 1 || io->kv_rows > rows_max)
            return ft_fail(ctx, FT_ERR_ARG, "ft_test_engine_handoffs: bad K/V layer, slot or row count");
        const FtLayer& l = fast ? ctx->flayers[io->kv_layer] : ctx->layers[io->kv_layer];
        const size_t mstr = fast ? ctx->fcache_m_stride : ctx->cache_m_stride;
        for (int h = 0; h < Hkv; ++h) {
            const size_t src = (size_t)io->kv_slot * mstr + (size_t)h * rows_max * hd, dst = (size_t)h * io->kv_rows * hd;
            const size_t bytes = (size_t)io->kv_rows * hd * esz;
            FT_HIP(ctx, hipMemcpy((char*)io->kv_k + dst * esz, (const char*)l.kc + src * esz, bytes, hipMemcpyDeviceToHost));
            FT_HIP(ctx, hipMemcpy((char*)io->kv_v + dst * esz, (const char*)l.vc + src * esz, bytes, hipMemcpyDeviceToHost));
        }
    }
    return FT_OK;
}

extern "C" ft_status ft_ar_park(ft_ctx* ctx, int32_t slot) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (slot < 0 || slot >= c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_park: bad slot");
    const int R = c.num_codebooks + 1;
    FT_TRY(ft_ar_reset(ctx, slot));
    // one stored frame = <|im_end|>, done = 1, a harmless input column (token 0, codes 0) at position 0
    int* h = ctx->h_pin;
    h[0] = c.im_end_id; h[1] = 1;
    FT_HIP(ctx, hipMemcpyAsync(ctx->d_seq + (size_t)slot * R * ctx->cap, h, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FT_HIP(ctx, hipMemcpyAsync(ctx->d_nf + slot, h + 1, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FT_HIP(ctx, hipMemcpyAsync(ctx->d_done + slot, h + 1, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FT_HIP(ctx, hipMemsetAsync(ctx->d_tok + (size_t)slot * R, 0, R * sizeof(int), ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FT_OK;
}

// ---- moving a live utterance to another slot (ft_ar_slot_move): ONE launch.  Workgroups [0, nkv) copy the slow stack's
// K/V rows [0, n_pos) of the slot, one workgroup per (layer, K | V, kv head, chunk of positions), in 16-byte pieces; the
// per-layer cache bases travel in the kernel's argument block (a table the kernel reads with scalar loads, as the frame
// engine reads its layer table).  The last workgroup (with `state` set) copies everything else a later frame of the slot
// reads - its row of the frame store (prompt and generated columns: the repetition-penalty window), position, input column,
// the column under construction, frame count, done flag and sampling row - and leaves `from` parked as ft_ar_park leaves it.
// Each element of `from` is read and rewritten by the same thread.  The codebook loop's K/V is rebuilt every frame.
constexpr int SLOT_MOVE_MAX_LAYERS = 64;     // cache bases per launch (deeper models: one launch per 64 layers)
struct SlotMoveP {
    char* kv[2 * SLOT_MOVE_MAX_LAYERS];   // [layer][K | V] cache bases of the layers of this launch
    size_t slot_bytes;       // one slot of one layer's K or V cache: Hkv x n_slots x hd elements
    size_t head_bytes;       // one kv head's cached positions: n_slots x hd elements
    int row16;               // 16-byte pieces per cached position (hd x esz / 16)
    int hkv, chunk, nchunk, nkv, n_pos, from, to, state;
    int *seq, *pos, *tok, *tokn, *nf, *done, *ctl;
    int seq_row, R, ctl_words, im_end;
};

static __global__ __launch_bounds__(256) void slot_move_kernel(SlotMoveP p) {
    const int b = blockIdx.x;
    if (b < p.nkv) {
        const int ci = b % p.nchunk, rest = b / p.nchunk;
        const int head = rest % p.hkv, lk = rest / p.hkv;
        const int p0 = ci * p.chunk, np = min(p.chunk, p.n_pos - p0);
        char* base = p.kv[lk] + (size_t)head * p.head_bytes + (size_t)p0 * p.row16 * 16;
        const U4* src = reinterpret_cast<const U4*>(base + (size_t)p.from * p.slot_bytes);
        U4* dst = reinterpret_cast<U4*>(base + (size_t)p.to * p.slot_bytes);
        const int n = np * p.row16;
        for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
        return;
    }
    if (!p.state) return;
    int* sf = p.seq + (size_t)p.from * p.seq_row;
    int* st = p.seq + (size_t)p.to * p.seq_row;
    for (int i = threadIdx.x; i < p.seq_row; i += blockDim.x) {
        const int v = sf[i];
        st[i] = v;
        sf[i] = i == 0 ? p.im_end : 0;      // parked: one stored frame = <|im_end|>
    }
    for (int i = threadIdx.x; i < p.R; i += blockDim.x) {
        const size_t f = (size_t)p.from * p.R + i, t = (size_t)p.to * p.R + i;
        const int a = p.tok[f], c = p.tokn[f];
        p.tok[t] = a; p.tokn[t] = c;
        p.tok[f] = 0;                       // parked: a harmless input column
    }
    for (int i = threadIdx.x; i < p.ctl_words; i += blockDim.x)
        p.ctl[(size_t)p.to * p.ctl_words + i] = p.ctl[(size_t)p.from * p.ctl_words + i];
    if (threadIdx.x == 0) {
        const int ps = p.pos[p.from], nf = p.nf[p.from], dn = p.done[p.from];
        p.pos[p.to] = ps; p.nf[p.to] = nf; p.done[p.to] = dn;
        p.pos[p.from] = 0; p.nf[p.from] = 1; p.done[p.from] = 1;
    }
}

// Between ft_ar_decode calls (and after a fill) only: the recovery of a frame-engine time-out needs nothing more here - it
// takes slot 0's position, frame count and done flag from the device at the start of every ft_ar_decode call (pos0, nf0,
// done0) and ft_ar_prefill_at / ft_ar_first_frames reset the slot they serve, so a moved utterance is rewound from its new
// slot like any other.  The host keeps one more piece of per-slot state, hid_in_xo (which buffer ft_ar_get_debug(hidden) reads
// the slot's residual stream from), and the move does not carry it - nor the hidden and logits rows themselves: those of `to`
// are defined again after its next frame, which sets the flag (include/fishtts_hip.h; tests/test_slot_state_gpu.py).
extern "C" ft_status ft_ar_slot_move(ft_ctx* ctx, int32_t from, int32_t to) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (from < 0 || from >= c.max_batch || to < 0 || to >= c.max_batch || from == to)
        return ft_fail(ctx, FT_ERR_ARG, "ft_ar_slot_move: bad slot (out of range, or from == to)");
    const int R = c.num_codebooks + 1;
    // the positions to carry: read behind every earlier call on the stream (an ft_ar_decode returns with it drained)
    FT_HIP(ctx, hipMemcpyAsync(ctx->h_pin, ctx->d_pos + from, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int n_pos = std::max(0, std::min(ctx->h_pin[0], ctx->n_slots));
    static_assert(sizeof(RowCtl) % sizeof(int) == 0, "the sampling row moves as whole words");
    SlotMoveP p{};
    p.slot_bytes = ctx->cache_m_stride * ctx->esz;
    p.head_bytes = (size_t)ctx->n_slots * c.head_dim * ctx->esz;
    p.row16 = (int)((size_t)c.head_dim * ctx->esz / 16);     // head_dim >= 8 (ar_validate): a position is >= 16 bytes
    p.hkv = c.n_local_heads;
    p.chunk = std::max(1, 1024 / p.row16);                    // ~16 KB per workgroup, four pieces per thread
    p.nchunk = std::max(1, (n_pos + p.chunk - 1) / p.chunk);
    p.n_pos = n_pos; p.from = from; p.to = to;
    p.seq = ctx->d_seq; p.pos = ctx->d_pos; p.tok = ctx->d_tok; p.tokn = ctx->d_tokn; p.nf = ctx->d_nf; p.done = ctx->d_done;
    p.ctl = reinterpret_cast<int*>(ctx->d_ctl);
    p.seq_row = R * ctx->cap; p.R = R; p.ctl_words = (int)(sizeof(RowCtl) / sizeof(int)); p.im_end = c.im_end_id;
    for (int l0 = 0; l0 < c.n_layer; l0 += SLOT_MOVE_MAX_LAYERS) {
        const int nl = std::min(SLOT_MOVE_MAX_LAYERS, c.n_layer - l0);
        for (int i = 0; i < nl; ++i) {
            p.kv[2 * i] = (char*)ctx->layers[l0 + i].kc;
            p.kv[2 * i + 1] = (char*)ctx->layers[l0 + i].vc;
        }
        p.nkv = n_pos > 0 ? 2 * nl * p.hkv * p.nchunk : 0;
        p.state = l0 + nl == c.n_layer;                      // the per-slot state moves with the last layers
        const int grid = p.nkv + (p.state ? 1 : 0);
        if (grid == 0) continue;
        slot_move_kernel<<<grid, 256, 0, ctx->stream>>>(p);
        FT_HIP(ctx, hipGetLastError());
    }
    return FT_OK;
}

extern "C" ft_status ft_ar_set_noise(ft_ctx* ctx, const float* q, int64_t n_rows, int64_t row_len) {
    if (!ctx || !ctx->has_ar) return FT_ERR_ARG;
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& kv : ctx->graphs) hipGraphExecDestroy(kv.second);  // captured launches hold the old pointer
    ctx->graphs.clear();
    if (ctx->noise) { hipFree(ctx->noise); ctx->noise = nullptr; }
    ctx->noise_rows = ctx->noise_row_len = 0;
    if (!q) return FT_OK;
    const int64_t need = (int64_t)ctx->c.vocab_size + (int64_t)(ctx->c.num_codebooks - 1) * ctx->fastV;
    if (row_len < need) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_set_noise: row_len too small");
    FT_HIP(ctx, hipMalloc((void**)&ctx->noise, (size_t)n_rows * row_len * sizeof(float)));
    FT_HIP(ctx, hipMemcpy(ctx->noise, q, (size_t)n_rows * row_len * sizeof(float), hipMemcpyDefault));
    ctx->noise_rows = n_rows;
    ctx->noise_row_len = row_len;
    return FT_OK;
}

extern "C" ft_status ft_ar_get_debug(ft_ctx* ctx, int32_t slot, float* logits, float* hidden) {
    FT_TRY(ar_ready(ctx));
    if (slot < 0 || slot >= ctx->c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "bad slot");
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (logits)
        FT_HIP(ctx, hipMemcpy(logits, ctx->logits + (size_t)slot * ctx->c.vocab_size, ctx->c.vocab_size * sizeof(float), hipMemcpyDeviceToHost));
    if (hidden && ctx->hid_in_xo[slot]) {
        // the slot's last frame ran on the MFMA launches: its residual stream is row `slot` of the octet-major xo_x (fast_dim ==
        // dim there), ctx->x holds what embed_kernel left
        const int D = ctx->c.dim;
        std::vector<uint16_t> hb((size_t)D);
        FT_HIP(ctx, hipMemcpy2D(hb.data(), 8 * sizeof(uint16_t), ctx->xo_x + (size_t)slot * 8, (size_t)ctx->xo_ldm * 8 * sizeof(uint16_t),
                                8 * sizeof(uint16_t), (size_t)D / 8, hipMemcpyDeviceToHost));
        for (int d = 0; d < D; ++d) {
            if (ctx->c.dtype == FT_BF16) { const uint32_t u = (uint32_t)hb[d] << 16; memcpy(hidden + d, &u, 4); }
            else { _Float16 v; memcpy(&v, &hb[d], 2); hidden[d] = (float)v; }
        }
    } else if (hidden)
        FT_HIP(ctx, hipMemcpy(hidden, ctx->hid + (size_t)slot * ctx->c.fast_dim, ctx->c.fast_dim * sizeof(float), hipMemcpyDeviceToHost));
    return FT_OK;
}

extern "C" ft_status ft_ar_profile_gemv(ft_ctx* ctx, int32_t frames, const ft_sampling* sp, double* ms,
                                        int64_t* launches, int64_t* bytes) {
    FT_TRY(ar_ready(ctx));
    if (!sp || !ms || !launches || !bytes) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_profile_gemv: null argument");
    const int R = ctx->c.num_codebooks + 1;
    FT_TRY(upload_ctl(ctx, 0, 1, sp));
    for (auto e : ctx->prof_ev) hipEventDestroy(e);
    ctx->prof_ev.clear();
    ctx->prof_bytes = ctx->prof_launches = 0;
    // The GEMV launches of one frame (weights of every layer in order, nothing else) are captured into a graph
    // and replayed `frames` times between two HIP events on the engine's stream: the average includes the
    // dependent-launch boundary exactly as rocprofv3's serialized kernel durations do.  The launch and byte
    // counters come from the same enqueue code as the real frame.
    double tot = 0.0;
    int64_t n_launch = 0, n_bytes = 0;
    bool graph_ok = true;
    if (graph_ok) {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
        Launch L{ctx, ctx->stream, 0, 1, 0};
        L.gemv_only = true;
        ctx->prof_count_only = true;
        ctx->prof = true;
        if (e == hipSuccess) {
            enqueue_frame(L, ctx->d_tok, 1, R, 0);
            e = hipStreamEndCapture(ctx->stream, &graph);
        }
        ctx->prof = false;
        ctx->prof_count_only = false;
        if (e == hipSuccess && L.err == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (graph) hipGraphDestroy(graph);
        graph_ok = e == hipSuccess && L.err == hipSuccess && exec != nullptr;
        if (graph_ok) {
            hipEvent_t e0, e1;
            hipEventCreate(&e0); hipEventCreate(&e1);
            hipGraphLaunch(exec, ctx->stream);  // warm
            hipEventRecord(e0, ctx->stream);
            for (int f = 0; f < frames; ++f) hipGraphLaunch(exec, ctx->stream);
            hipEventRecord(e1, ctx->stream);
            graph_ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
            float t = 0.f;
            if (graph_ok) graph_ok = hipEventElapsedTime(&t, e0, e1) == hipSuccess;
            tot = t;
            n_launch = ctx->prof_launches * frames;
            n_bytes = ctx->prof_bytes * frames;
            hipEventDestroy(e0); hipEventDestroy(e1);
        }
        if (exec) hipGraphExecDestroy(exec);
        (void)hipGetLastError();
    }
    if (!graph_ok) {
        for (auto e : ctx->prof_ev) hipEventDestroy(e);
        ctx->prof_ev.clear();
        ctx->prof_bytes = ctx->prof_launches = 0;
        tot = 0.0;
        ctx->prof = true;
        for (int f = 0; f < frames; ++f) {
            Launch L{ctx, ctx->stream, 0, 1, 0};
            enqueue_frame(L, ctx->d_tok, 1, R, 0);
            if (L.err != hipSuccess) { ctx->prof = false; return ft_fail(ctx, FT_ERR_HIP, "profile launch failed"); }
        }
        ctx->prof = false;
        FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i + 1 < ctx->prof_ev.size(); i += 2) {
            float t = 0.f;
            hipEventElapsedTime(&t, ctx->prof_ev[i], ctx->prof_ev[i + 1]);
            tot += t;
        }
        n_launch = ctx->prof_launches;
        n_bytes = ctx->prof_bytes;
    }
    *ms = tot; *launches = n_launch; *bytes = n_bytes;
    for (auto e : ctx->prof_ev) hipEventDestroy(e);
    ctx->prof_ev.clear();
    return FT_OK;
}

extern "C" ft_status ft_ar_profile_frame(ft_ctx* ctx, int32_t frames, const ft_sampling* sp, double* ms_graph,
                                         double* seg_ms, int32_t* nodes_per_frame) {
    FT_TRY(ar_ready(ctx));
    if (!sp || frames < 1) return ft_fail(ctx, FT_ERR_ARG, "ft_ar_profile_frame: bad argument");
    const ft_ar_config& c = ctx->c;
    const int R = c.num_codebooks + 1;
    FT_TRY(upload_ctl(ctx, 0, 1, sp));
    int h[2] = {0, 0};
    FT_HIP(ctx, hipMemcpy(h, ctx->d_nf, sizeof(int), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(h + 1, ctx->d_pos, sizeof(int), hipMemcpyDeviceToHost));
    if (h[0] < 1) return ft_fail(ctx, FT_ERR_STATE, "ft_ar_profile_frame: slot 0 has not been prefilled");
    if (h[0] + 2 * frames + 2 > ctx->cap || h[1] + 2 * frames + 2 > ctx->n_slots)
        return ft_fail(ctx, FT_ERR_ARG, "ft_ar_profile_frame: not enough frame / cache capacity left in slot 0");
    hipEvent_t ev[4];
    for (auto& e : ev) FT_HIP(ctx, hipEventCreate(&e));
    // (1) the captured frame graph, replayed back to back
    hipGraphExec_t exec = nullptr;
    FT_TRY(get_graph(ctx, 1, &exec));
    FT_HIP(ctx, hipGraphLaunch(exec, ctx->stream));
    FT_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    for (int f = 0; f < frames; ++f) FT_HIP(ctx, hipGraphLaunch(exec, ctx->stream));
    FT_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float t = 0.f;
    FT_HIP(ctx, hipEventElapsedTime(&t, ev[0], ev[1]));
    if (ms_graph) *ms_graph = t;
    if (nodes_per_frame) { auto it = ctx->graph_nodes.find(graph_key(ctx, 1, 1)); *nodes_per_frame = it == ctx->graph_nodes.end() ? 0 : it->second; }
    // (2) the same frame launched eagerly, events between its three parts (bf16 only)
    double seg[3] = {0, 0, 0};
    if (seg_ms && c.dtype == FT_BF16) {
        for (int f = 0; f < frames - 1; ++f) {
            Launch L{ctx, ctx->stream, 0, 1, 0};
            FT_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
            if (eng_slow_ok(L)) enqueue_slow_engine(L, ctx->d_tok, 1, R, 0);
            else enqueue_slow<bf16_t, RND_BF16>(L, ctx->d_tok, 1, R, 0, true);
            FT_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
            enqueue_head<bf16_t, RND_BF16>(L);
            enqueue_sample<bf16_t, RND_BF16>(L, 0, c.num_codebooks == 1);
            FT_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
            if (eng_fast_ok(L)) enqueue_fast_engine(L);
            else for (int cb = 0; cb < c.num_codebooks; ++cb) enqueue_fast_step<bf16_t, RND_BF16>(L, cb);
            FT_HIP(ctx, hipEventRecord(ev[3], ctx->stream));
            FT_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (L.err != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_ar_profile_frame: launch failed");
            for (int k = 0; k < 3; ++k) { float d = 0.f; hipEventElapsedTime(&d, ev[k], ev[k + 1]); seg[k] += d; }
        }
        for (int k = 0; k < 3; ++k) seg_ms[k] = seg[k];
    } else if (seg_ms) {
        seg_ms[0] = seg_ms[1] = seg_ms[2] = 0.0;
    }
    for (auto& e : ev) hipEventDestroy(e);
    bool aborted = false;
    FT_TRY(eng_recover(ctx, &aborted));
    if (aborted) return ft_fail(ctx, FT_ERR_HIP, "ft_ar_profile_frame: a frame-engine hand-off timed out; the timing is invalid");
    return FT_OK;
}

extern "C" ft_status ft_test_sample(ft_ctx* ctx, const float* logits, int32_t cb, const ft_sampling* sp,
                                    const int32_t* window, const float* q, int32_t* out_index) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (!logits || !sp || !out_index || cb < 0 || cb >= c.num_codebooks) return ft_fail(ctx, FT_ERR_ARG, "ft_test_sample: bad argument");
    const int R = c.num_codebooks + 1;
    const int V = cb == 0 ? c.vocab_size : ctx->fastV;
    FT_TRY(ft_ar_reset(ctx, 0));
    FT_TRY(upload_ctl(ctx, 0, 1, sp));
    FT_HIP(ctx, hipMemcpy(cb == 0 ? ctx->logits : ctx->flog, logits, (size_t)V * sizeof(float), hipMemcpyHostToDevice));
    int nfv = 0;
    if (window) {
        nfv = 1;  // iteration i = 0: the window is hist[:, 0:16] = seq[:, 1:17]
        for (int r = 0; r < R; ++r)
            FT_HIP(ctx, hipMemcpy(ctx->d_seq + (size_t)r * ctx->cap + 1, window + (size_t)r * 16, 16 * sizeof(int), hipMemcpyHostToDevice));
        FT_HIP(ctx, hipMemcpy(ctx->d_nf, &nfv, sizeof(int), hipMemcpyHostToDevice));
    }
    float* saved = ctx->noise;
    const long srows = ctx->noise_rows, slen = ctx->noise_row_len;
    float* tmp = nullptr;
    if (q) {
        const long need = (long)c.vocab_size + (long)(c.num_codebooks - 1) * ctx->fastV;
        FT_HIP(ctx, hipMalloc((void**)&tmp, (size_t)(nfv + 1) * need * sizeof(float)));
        const long off = cb == 0 ? 0 : (long)c.vocab_size + (long)(cb - 1) * ctx->fastV;
        FT_HIP(ctx, hipMemcpy(tmp + (size_t)nfv * need + off, q, (size_t)V * sizeof(float), hipMemcpyHostToDevice));
        ctx->noise = tmp; ctx->noise_rows = nfv + 1; ctx->noise_row_len = need;
    } else {
        ctx->noise = nullptr; ctx->noise_rows = 0;
    }
    Launch L{ctx, ctx->stream, 0, 1, 0};
    by_dtype(ctx, [&](auto t) { using T = decltype(t); return enqueue_sample<typename T::WT, T::ROUND>(L, cb, false); });
    hipError_t e = hipStreamSynchronize(ctx->stream);
    ctx->noise = saved; ctx->noise_rows = srows; ctx->noise_row_len = slen;
    if (tmp) hipFree(tmp);
    if (L.err != hipSuccess || e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_sample launch failed");
    int tokn[2] = {0, 0};
    FT_HIP(ctx, hipMemcpy(tokn, ctx->d_tokn + (cb == 0 ? 0 : cb + 1), sizeof(int), hipMemcpyDeviceToHost));
    *out_index = tokn[0];
    return ft_ar_reset(ctx, 0);
}

// device temporaries and sentinels of the test hooks below
namespace {
constexpr uint16_t WT_POISON = 0xFFFE;          // a NaN in bf16 and in fp16: operand rows >= M, and the 16-bit output sentinel
constexpr uint32_t WT_POISON_F32 = 0xFFFFFFFEu; // the f32 output sentinel (a NaN)
struct DevTmp {                                  // device temporaries of one hook call
    std::vector<void*> v;
    ~DevTmp() { for (void* p : v) hipFree(p); }
    void* put(const void* host, size_t bytes) {
        void* d = nullptr;
        if (hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) return nullptr;
        v.push_back(d);
        if (host && bytes && hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
};
}  // namespace

// Test hook (include/fishtts_hip_test.h: ft_test_draw): ONE enqueue_sample on the context's own buffers, M rows, every
// buffer the draw may write pre-filled and returned whole.  Host code only: nothing here is reached from a frame.
static ft_status test_draw_run(ft_ctx* ctx, ft_test_draw_io* io);
extern "C" ft_status ft_test_draw(ft_ctx* ctx, ft_test_draw_io* io) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (!io) return ft_fail(ctx, FT_ERR_ARG, "ft_test_draw: no argument block");
    const int MB = c.max_batch, M = io->M, cb = io->cb, R = c.num_codebooks + 1;
    if (M < 1 || M > MB) return ft_fail(ctx, FT_ERR_ARG, "ft_test_draw: M outside 1..max_batch");
    if (cb < 0 || cb >= c.num_codebooks) return ft_fail(ctx, FT_ERR_ARG, "ft_test_draw: bad codebook");
    if (io->last != 0 && io->last != 1) return ft_fail(ctx, FT_ERR_ARG, "ft_test_draw: last is 0 or 1");
    if (!io->logits || !io->sp || !io->tokn || !io->tok || !io->seq || !io->pos || !io->nf || !io->done || !io->logits_out ||
        !io->femb || !io->qkvf || !io->cut || !io->chunk_cnt || !io->part_idx || (ctx->wide_ok && (!io->xo_femb || !io->xo_x)))
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_draw: missing argument");
    const long need = (long)c.vocab_size + (long)(c.num_codebooks - 1) * ctx->fastV;
    if (io->noise && (io->noise_rows < 1 || io->noise_row_len < need))
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_draw: noise block smaller than one frame's draws");
    for (int m = 0; m < M; ++m)      // the kernels index the history and the noise by nf: keep both inside their blocks
        if (io->nf[m] < 0 || io->nf[m] > ctx->cap || (io->noise && io->nf[m] >= io->noise_rows))
            return ft_fail(ctx, FT_ERR_ARG, "ft_test_draw: nf outside 0..cap or past the noise block");
    // the device work, then - whatever it returned - the context's own noise back and every slot as a reset leaves it
    float* saved = ctx->noise;
    const long srows = ctx->noise_rows, slen = ctx->noise_row_len;
    const ft_status st = test_draw_run(ctx, io);
    ctx->noise = saved; ctx->noise_rows = srows; ctx->noise_row_len = slen;
    (void)hipStreamSynchronize(ctx->stream);
    if (st != FT_OK) (void)hipGetLastError();
    bool ok = hipMemsetAsync(ctx->d_tokn, 0, (size_t)MB * R * sizeof(int), ctx->stream) == hipSuccess &&
              hipMemsetAsync(ctx->d_tok, 0, (size_t)MB * R * sizeof(int), ctx->stream) == hipSuccess;
    for (int m = 0; m < MB; ++m) ok = ft_ar_reset(ctx, m) == FT_OK && ok;
    ok = hipStreamSynchronize(ctx->stream) == hipSuccess && ok;
    if (st != FT_OK) return st;
    return ok ? FT_OK : ft_fail(ctx, FT_ERR_HIP, "ft_test_draw: reset failed");
}

static ft_status test_draw_run(ft_ctx* ctx, ft_test_draw_io* io) {
    const ft_ar_config& c = ctx->c;
    const int MB = c.max_batch, M = io->M, cb = io->cb, R = c.num_codebooks + 1;
    const int V = cb == 0 ? c.vocab_size : ctx->fastV;
    const size_t fqkvN = (size_t)(c.fast_n_head + 2 * c.fast_n_local_heads) * c.fast_head_dim;
    const size_t qkvf_n = 2 * (((size_t)MB + 15) / 16 * 16) * fqkvN;
    const size_t nchunk = ((size_t)c.vocab_size + 1023) / 1024;
    const size_t xo_n = ctx->wide_ok ? (size_t)ctx->xo_ldm * c.dim : 0;     // wide_ok: fast_dim == dim
    float* dl = cb == 0 ? ctx->logits : ctx->flog;
    hipStream_t st = ctx->stream;
    // 0xFF bytes: a NaN in f32, bf16 and fp16, -1 in the integer scratch
    FT_HIP(ctx, hipMemsetAsync(dl, 0xFF, (size_t)MB * V * sizeof(float), st));
    FT_HIP(ctx, hipMemsetAsync(ctx->femb, 0xFF, (size_t)MB * c.fast_dim * sizeof(float), st));
    FT_HIP(ctx, hipMemsetAsync(ctx->qkvf, 0xFF, qkvf_n * sizeof(float), st));
    FT_HIP(ctx, hipMemsetAsync(ctx->d_ctl, 0xFF, (size_t)MB * sizeof(RowCtl), st));
    FT_HIP(ctx, hipMemsetAsync(ctx->samp_cut, 0xFF, (size_t)MB * sizeof(SampCut), st));
    FT_HIP(ctx, hipMemsetAsync(ctx->samp_chunk_cnt, 0xFF, MB * nchunk * sizeof(int), st));
    FT_HIP(ctx, hipMemsetAsync(ctx->samp_part_score, 0xFF, MB * nchunk * sizeof(float), st));
    FT_HIP(ctx, hipMemsetAsync(ctx->samp_part_idx, 0xFF, MB * nchunk * sizeof(int), st));
    if (xo_n) {
        FT_HIP(ctx, hipMemsetAsync(ctx->xo_femb, 0xFF, xo_n * sizeof(bf16_t), st));
        FT_HIP(ctx, hipMemsetAsync(ctx->xo_x, 0xFF, xo_n * sizeof(bf16_t), st));
    }
    FT_HIP(ctx, hipStreamSynchronize(st));
    FT_TRY(upload_ctl(ctx, 0, M, io->sp));
    FT_HIP(ctx, hipMemcpy(dl, io->logits, (size_t)M * V * sizeof(float), hipMemcpyHostToDevice));
    FT_HIP(ctx, hipMemcpy(ctx->d_tokn, io->tokn, (size_t)MB * R * sizeof(int), hipMemcpyHostToDevice));
    FT_HIP(ctx, hipMemcpy(ctx->d_tok, io->tok, (size_t)MB * R * sizeof(int), hipMemcpyHostToDevice));
    FT_HIP(ctx, hipMemcpy(ctx->d_seq, io->seq, (size_t)MB * R * ctx->cap * sizeof(int), hipMemcpyHostToDevice));
    FT_HIP(ctx, hipMemcpy(ctx->d_pos, io->pos, (size_t)MB * sizeof(int), hipMemcpyHostToDevice));
    FT_HIP(ctx, hipMemcpy(ctx->d_nf, io->nf, (size_t)MB * sizeof(int), hipMemcpyHostToDevice));
    FT_HIP(ctx, hipMemcpy(ctx->d_done, io->done, (size_t)MB * sizeof(int), hipMemcpyHostToDevice));
    DevTmp tmp;
    if (io->noise) {
        float* dq = (float*)tmp.put(io->noise, (size_t)io->noise_rows * io->noise_row_len * sizeof(float));
        if (!dq) { (void)hipGetLastError(); return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_draw: noise block"); }
        ctx->noise = dq; ctx->noise_rows = io->noise_rows; ctx->noise_row_len = io->noise_row_len;
    } else {
        ctx->noise = nullptr; ctx->noise_rows = 0;
    }
    Launch L{ctx, st, 0, M, 0};
    const int what = by_dtype(ctx, [&](auto t) { using T = decltype(t); return enqueue_sample<typename T::WT, T::ROUND>(L, cb, io->last != 0); });
    hipError_t e = hipStreamSynchronize(st);
    if (L.err != hipSuccess || e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_draw launch failed");
    io->what = what;
    FT_HIP(ctx, hipMemcpy(io->logits_out, dl, (size_t)MB * V * sizeof(float), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->tokn, ctx->d_tokn, (size_t)MB * R * sizeof(int), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->tok, ctx->d_tok, (size_t)MB * R * sizeof(int), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->seq, ctx->d_seq, (size_t)MB * R * ctx->cap * sizeof(int), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->pos, ctx->d_pos, (size_t)MB * sizeof(int), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->nf, ctx->d_nf, (size_t)MB * sizeof(int), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->done, ctx->d_done, (size_t)MB * sizeof(int), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->femb, ctx->femb, (size_t)MB * c.fast_dim * sizeof(float), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->qkvf, ctx->qkvf, qkvf_n * sizeof(float), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->cut, ctx->samp_cut, (size_t)MB * sizeof(SampCut), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->chunk_cnt, ctx->samp_chunk_cnt, MB * nchunk * sizeof(int), hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(io->part_idx, ctx->samp_part_idx, MB * nchunk * sizeof(int), hipMemcpyDeviceToHost));
    if (xo_n) {
        FT_HIP(ctx, hipMemcpy(io->xo_femb, ctx->xo_femb, xo_n * sizeof(bf16_t), hipMemcpyDeviceToHost));
        FT_HIP(ctx, hipMemcpy(io->xo_x, ctx->xo_x, xo_n * sizeof(bf16_t), hipMemcpyDeviceToHost));
    }
    return FT_OK;
}

// Test hook: rows [row0, row0 + rows) of the lock-step batches' layer-0 q k v table as raw 16-bit patterns; *present = 0 (out
// untouched) on a context that built none.
extern "C" ft_status ft_test_qkv0_tab(ft_ctx* ctx, int32_t row0, int32_t rows, uint16_t* out, int32_t* present) {
    FT_TRY(ar_ready(ctx));
    if (!present) return ft_fail(ctx, FT_ERR_ARG, "ft_test_qkv0_tab: missing argument");
    *present = ctx->wide_qkv0_tab ? 1 : 0;
    if (!ctx->wide_qkv0_tab) return FT_OK;
    const ft_ar_config& c = ctx->c;
    const size_t n = (size_t)(c.fast_n_head + 2 * c.fast_n_local_heads) * c.fast_head_dim;
    if (!out || row0 < 0 || rows < 1 || (long)row0 + rows > ctx->fastV) return ft_fail(ctx, FT_ERR_ARG, "ft_test_qkv0_tab: bad row range");
    FT_HIP(ctx, hipMemcpy(out, ctx->wide_qkv0_tab + (size_t)row0 * n, (size_t)rows * n * sizeof(bf16_t), hipMemcpyDeviceToHost));
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ lock-step kernel test hooks
// (include/fishtts_hip_test.h: ft_test_wide_linear, ft_test_wide_attn).  Host code around the product's own dispatchers
// wide_gemm and wide_attn on temporaries: nothing here is reached from a frame.

template <typename WT>
static ft_status test_wide_linear_t(ft_ctx* ctx, int epi, bool vocab_head, int M, int N, int K, const uint16_t* X, const uint16_t* W,
                                    const uint16_t* gain, const float* bias, const uint16_t* resid, bool alias, void* out,
                                    void* out_tail, int32_t* tail_rows, int32_t* variant) {
    const int ldm = ctx->xo_ldm;
    const int Mt = (M + 31) / 32 * 32;           // the edge of the tallest batch tile (TS = 2); <= ldm, a multiple of 32
    const int oc = epi == WEPI_SWIGLU ? N / 2 : N;
    auto to_xo = [&](const uint16_t* rows, int width) {
        std::vector<uint16_t> o((size_t)width * ldm, WT_POISON);
        for (int m = 0; m < M; ++m)
            for (int k = 0; k < width; ++k) o[xo_index(m, k, ldm)] = rows[(size_t)m * width + k];
        return o;
    };
    DevTmp tmp;
    const std::vector<uint16_t> xo = to_xo(X, K);
    void* dX = tmp.put(xo.data(), xo.size() * 2);
    void* dW = tmp.put(W, (size_t)N * K * 2);
    void* dG = gain ? tmp.put(gain, (size_t)K * 2) : nullptr;
    void* dB = bias ? tmp.put(bias, (size_t)N * sizeof(float)) : nullptr;
    void *dO = nullptr, *dR = nullptr;
    if (epi == WEPI_STORE) {
        const std::vector<uint32_t> fill((size_t)Mt * N, WT_POISON_F32);
        dO = tmp.put(fill.data(), fill.size() * 4);
    } else {
        const std::vector<uint16_t> fill((size_t)oc * ldm, WT_POISON);
        if (epi == WEPI_RESID) {
            const std::vector<uint16_t> ro = to_xo(resid, N);
            dR = tmp.put(ro.data(), ro.size() * 2);
            dO = alias ? dR : tmp.put(fill.data(), fill.size() * 2);
        } else {
            dO = tmp.put(fill.data(), fill.size() * 2);
        }
    }
    if (!dX || !dW || (gain && !dG) || (bias && !dB) || !dO || (epi == WEPI_RESID && !dR)) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_wide_linear: device temporaries");
    }
    Launch L{ctx, ctx->stream, 0, M, 0};
    const int id = wide_gemm<WT>(L, (const bf16_t*)dX, dW, (const float*)dB, N, K, dG, epi, epi == WEPI_STORE ? (float*)dO : nullptr, (long)N,
                                 epi == WEPI_STORE ? nullptr : (bf16_t*)dO, (const bf16_t*)dR, M, vocab_head);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (L.err == hipErrorInvalidValue) return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_linear: N is not a whole number of the launch's tiles");
    if (L.err != hipSuccess || e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_wide_linear launch failed");
    if (epi == WEPI_STORE) {
        std::vector<float> o((size_t)Mt * N);
        FT_HIP(ctx, hipMemcpy(o.data(), dO, o.size() * 4, hipMemcpyDeviceToHost));
        memcpy(out, o.data(), (size_t)M * N * 4);
        memcpy(out_tail, o.data() + (size_t)M * N, (size_t)(Mt - M) * N * 4);
    } else {
        std::vector<uint16_t> o((size_t)oc * ldm);
        FT_HIP(ctx, hipMemcpy(o.data(), dO, o.size() * 2, hipMemcpyDeviceToHost));
        for (int m = 0; m < Mt; ++m) {
            uint16_t* dst = m < M ? (uint16_t*)out + (size_t)m * oc : (uint16_t*)out_tail + (size_t)(m - M) * oc;
            for (int k = 0; k < oc; ++k) dst[k] = o[xo_index(m, k, ldm)];
        }
    }
    *tail_rows = Mt - M;
    *variant = id;
    return FT_OK;
}

extern "C" ft_status ft_test_wide_linear(ft_ctx* ctx, int32_t epi, int32_t vocab_head, int32_t M, int32_t N, int32_t K,
                                         const uint16_t* X, const uint16_t* W, const uint16_t* gain, const float* bias,
                                         const uint16_t* resid, int32_t alias, void* out, void* out_tail, int32_t* tail_rows,
                                         int32_t* variant) {
    FT_TRY(ar_ready(ctx));
    if (ctx->c.dtype != FT_BF16 && ctx->c.dtype != FT_F16) return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_linear: the model's type is not 16-bit");
    if (!ctx->wide_ok) return ft_fail(ctx, FT_ERR_STATE, "ft_test_wide_linear: this context has no lock-step MFMA path");
    if (epi != WEPI_STORE && epi != WEPI_SWIGLU && epi != WEPI_RESID) return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_linear: bad epilogue");
    if (M < 1 || M > ctx->xo_ldm) return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_linear: M outside 1..xo_ldm");
    if (!wide_k_ok(K)) return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_linear: K must be 1024, 2048 or 3072");
    if (N < 16 || N % 16 != 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_linear: N is not a whole number of 16-row tiles");
    if (!X || !W || !out || !out_tail || !tail_rows || !variant || (epi != WEPI_RESID && !gain) || (epi == WEPI_RESID && !resid))
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_linear: missing argument");
    if (ctx->c.dtype == FT_BF16)
        return test_wide_linear_t<bf16_t>(ctx, epi, vocab_head != 0, M, N, K, X, W, epi == WEPI_RESID ? nullptr : gain, bias, resid, alias != 0, out, out_tail, tail_rows, variant);
    return test_wide_linear_t<f16_t>(ctx, epi, vocab_head != 0, M, N, K, X, W, epi == WEPI_RESID ? nullptr : gain, bias, resid, alias != 0, out, out_tail, tail_rows, variant);
}

template <typename WT, int ROUND>
static ft_status test_wide_attn_t(ft_ctx* ctx, int M, const float* qkv, const int32_t* pos, const uint16_t* qn, const uint16_t* kn,
                                  uint16_t* kc, uint16_t* vc, uint16_t* y, int32_t* splits) {
    const ft_ar_config& c = ctx->c;
    const int HD = c.n_head * c.head_dim, ldm = ctx->xo_ldm;
    const size_t qkvN = (size_t)(c.n_head + 2 * c.n_local_heads) * c.head_dim;
    const size_t cbytes = (size_t)M * ctx->cache_m_stride * 2;
    DevTmp tmp;
    const std::vector<uint16_t> fill((size_t)HD * ldm, WT_POISON);
    void* dQ = tmp.put(qkv, (size_t)M * qkvN * sizeof(float));
    void* dP = tmp.put(pos, (size_t)M * sizeof(int));
    void* dQn = tmp.put(qn, (size_t)c.head_dim * 2);
    void* dKn = tmp.put(kn, (size_t)c.head_dim * 2);
    void* dK = tmp.put(kc, cbytes);
    void* dV = tmp.put(vc, cbytes);
    void* dY = tmp.put(fill.data(), fill.size() * 2);
    if (!dQ || !dP || !dQn || !dKn || !dK || !dV || !dY) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_wide_attn: device temporaries");
    }
    Launch L{ctx, ctx->stream, 0, M, 0};
    AttnP a{};
    a.qkv = (const float*)dQ; a.ldq = (int)qkvN; a.qn = dQn; a.kn = dKn; a.rope = ctx->rope;
    a.kc = dK; a.vc = dV; a.cache_m_stride = ctx->cache_m_stride; a.pos = (const int*)dP; a.pos_off = 0;
    a.H = c.n_head; a.Hkv = c.n_local_heads; a.hd = c.head_dim; a.n_slots = ctx->n_slots;
    a.eps = c.norm_eps; a.scale = 1.0f / sqrtf((float)c.head_dim);
    a.y = nullptr; a.ldy = HD; a.y_bf = (bf16_t*)dY; a.y_xo_ldm = ldm;
    *splits = wide_attn<WT, ROUND>(L, a);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (L.err != hipSuccess || e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_wide_attn launch failed");
    std::vector<uint16_t> o((size_t)HD * ldm);
    FT_HIP(ctx, hipMemcpy(o.data(), dY, o.size() * 2, hipMemcpyDeviceToHost));
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < HD; ++k) y[(size_t)m * HD + k] = o[xo_index(m, k, ldm)];
    FT_HIP(ctx, hipMemcpy(kc, dK, cbytes, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(vc, dV, cbytes, hipMemcpyDeviceToHost));
    return FT_OK;
}

extern "C" ft_status ft_test_wide_attn(ft_ctx* ctx, int32_t M, const float* qkv, const int32_t* pos, const uint16_t* qn,
                                       const uint16_t* kn, uint16_t* kc, uint16_t* vc, uint16_t* y, int32_t* splits) {
    FT_TRY(ar_ready(ctx));
    if (ctx->c.dtype != FT_BF16 && ctx->c.dtype != FT_F16) return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_attn: the model's type is not 16-bit");
    if (!ctx->wide_ok) return ft_fail(ctx, FT_ERR_STATE, "ft_test_wide_attn: this context has no lock-step MFMA path");
    if (M < 1 || M > ctx->c.max_batch || M > 64) return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_attn: M outside 1..min(max_batch, 64)");
    if (!qkv || !pos || !qn || !kn || !kc || !vc || !y || !splits) return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_attn: missing argument");
    for (int m = 0; m < M; ++m)
        if (pos[m] < 0 || pos[m] >= ctx->n_slots || pos[m] >= ctx->c.max_seq_len)
            return ft_fail(ctx, FT_ERR_ARG, "ft_test_wide_attn: a position outside the cache or the rope table");
    if (ctx->c.dtype == FT_BF16) return test_wide_attn_t<bf16_t, RND_BF16>(ctx, M, qkv, pos, qn, kn, kc, vc, y, splits);
    return test_wide_attn_t<f16_t, RND_F16>(ctx, M, qkv, pos, qn, kn, kc, vc, y, splits);
}

// ------------------------------------------------------------------------------------------ prompt-pass kernel test hooks
// (include/fishtts_hip_test.h: ft_test_pf_linear, ft_test_pf_norm, ft_test_pf_attn).  Host code around pf_gemm, the row norm
// and pf_attn on temporaries: nothing here is reached from a prompt pass.
static ft_status pf_hook_ready(ft_ctx* ctx, const char* who) {
    FT_TRY(ar_ready(ctx));
    if (ctx->c.dtype != FT_BF16) return ft_fail(ctx, FT_ERR_ARG, std::string(who) + ": the MFMA prompt pass is bf16 only");
    if (ctx->prefill_v0) return ft_fail(ctx, FT_ERR_STATE, std::string(who) + ": this context runs its prompts position by position");
    return FT_OK;
}

extern "C" ft_status ft_test_pf_linear(ft_ctx* ctx, int32_t form, int32_t S, int32_t N, int32_t K, const uint16_t* X,
                                       const uint16_t* W, const float* bias, const float* resid, int32_t alias, void* out,
                                       void* out_tail, int32_t* tail_rows, int32_t* variant) {
    FT_TRY(pf_hook_ready(ctx, "ft_test_pf_linear"));
    if (form < 0 || form > 2) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_linear: bad form");
    if (S < 1 || S > ctx->c.max_seq_len) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_linear: S outside 1..max_seq_len");
    if (K < 32 || K % 32 != 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_linear: K is not a whole number of 32-wide MFMA steps");
    if (N < 16 || N % 16 != 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_linear: N is not a whole number of 16-row tiles");
    if (!X || !W || !out || !out_tail || !tail_rows || !variant || (form == 1 && !resid))
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_linear: missing argument");
    const int St = (S + 127) / 128 * 128;          // the edge of the tallest row tile of any class
    const int oc = form == 2 ? N / 2 : N;
    DevTmp tmp;
    std::vector<uint16_t> xh((size_t)St * K, WT_POISON);
    memcpy(xh.data(), X, (size_t)S * K * 2);
    void* dX = tmp.put(xh.data(), xh.size() * 2);
    void* dW = tmp.put(W, (size_t)N * K * 2);
    void* dB = bias ? tmp.put(bias, (size_t)N * sizeof(float)) : nullptr;
    void *dO = nullptr, *dR = nullptr;
    if (form == 2) {
        const std::vector<uint16_t> fill((size_t)St * oc, WT_POISON);
        dO = tmp.put(fill.data(), fill.size() * 2);
    } else {
        std::vector<uint32_t> fill((size_t)St * N, WT_POISON_F32);
        if (form == 1) {
            std::vector<uint32_t> rh = fill;       // residual rows S .. St - 1 hold the sentinel too (the in-place form returns them)
            memcpy(rh.data(), resid, (size_t)S * N * 4);
            dR = tmp.put(rh.data(), rh.size() * 4);
        }
        dO = form == 1 && alias ? dR : tmp.put(fill.data(), fill.size() * 4);
    }
    if (!dX || !dW || (bias && !dB) || !dO || (form == 1 && !dR)) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_pf_linear: device temporaries");
    }
    Launch L{ctx, ctx->stream, 0, 1, 0};
    int id;
    if (form == 0) id = pf_gemm(L, (const bf16_t*)dX, K, S, dW, (const float*)dB, N, K, ACT_NONE, nullptr, (float*)dO, nullptr, N, 0);
    else if (form == 1) id = pf_gemm(L, (const bf16_t*)dX, K, S, dW, (const float*)dB, N, K, ACT_NONE, (const float*)dR, (float*)dO, nullptr, N, 1);
    else id = pf_gemm(L, (const bf16_t*)dX, K, S, dW, (const float*)dB, N, K, ACT_SWIGLU, nullptr, nullptr, (bf16_t*)dO, oc, 0);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (L.err != hipSuccess || e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_pf_linear launch failed");
    const size_t esz = form == 2 ? 2 : 4;
    std::vector<char> o((size_t)St * oc * esz);
    FT_HIP(ctx, hipMemcpy(o.data(), dO, o.size(), hipMemcpyDeviceToHost));
    memcpy(out, o.data(), (size_t)S * oc * esz);
    memcpy(out_tail, o.data() + (size_t)S * oc * esz, (size_t)(St - S) * oc * esz);
    *tail_rows = St - S;
    *variant = id;
    return FT_OK;
}

extern "C" ft_status ft_test_pf_norm(ft_ctx* ctx, int32_t S, int32_t D, const float* x, const uint16_t* gain, uint16_t* out,
                                     uint16_t* out_tail) {
    FT_TRY(pf_hook_ready(ctx, "ft_test_pf_norm"));
    if (S < 1 || S > ctx->c.max_seq_len || D < 1) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_norm: S outside 1..max_seq_len or D < 1");
    if (!x || !gain || !out || !out_tail) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_norm: missing argument");
    DevTmp tmp;
    const std::vector<uint16_t> fill((size_t)(S + 1) * D, WT_POISON);
    void* dX = tmp.put(x, (size_t)S * D * sizeof(float));
    void* dG = tmp.put(gain, (size_t)D * 2);
    void* dO = tmp.put(fill.data(), fill.size() * 2);
    if (!dX || !dG || !dO) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_pf_norm: device temporaries");
    }
    rmsnorm_llama_rows_kernel<bf16_t, true><<<S, 256, 0, ctx->stream>>>((const float*)dX, dG, ctx->c.norm_eps, D, (bf16_t*)dO);
    const hipError_t le = hipGetLastError(), e = hipStreamSynchronize(ctx->stream);
    if (le != hipSuccess || e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_pf_norm launch failed");
    FT_HIP(ctx, hipMemcpy(out, dO, (size_t)S * D * 2, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(out_tail, (const uint16_t*)dO + (size_t)S * D, (size_t)D * 2, hipMemcpyDeviceToHost));
    return FT_OK;
}

extern "C" ft_status ft_test_pf_attn(ft_ctx* ctx, int32_t n_seq, const int32_t* seqs, int32_t Lp, int32_t pos0, int32_t slot,
                                     const float* qkv, const uint16_t* qn, const uint16_t* kn, uint16_t* kc, uint16_t* vc,
                                     uint16_t* y, uint16_t* q, uint16_t* tail, int32_t* path) {
    FT_TRY(pf_hook_ready(ctx, "ft_test_pf_attn"));
    const ft_ar_config& c = ctx->c;
    if (!qkv || !qn || !kn || !kc || !vc || !y || !q || !tail || !path || (n_seq > 0 && !seqs))
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_attn: missing argument");
    if (n_seq < 0 || n_seq > c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_attn: bad sequence count");
    std::vector<int4> sq;
    std::vector<int2> rows;
    int S = 0, max_lp = 0;
    if (n_seq == 0) {
        if (slot < 0 || slot >= c.max_batch || Lp < 1 || pos0 < 0 || pos0 + Lp >= c.max_seq_len)
            return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_attn: bad slot, empty prompt or a prompt past max_seq_len");
        sq.push_back(int4{0, Lp, pos0, slot});
        S = max_lp = Lp;
    } else {
        if ((c.head_dim != 64 && c.head_dim != 128) || getenv("FT_PREFILL_ATTN_V0"))
            return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_attn: a ragged pass runs on the tiled kernel only");
        std::vector<char> seen(c.max_batch, 0);
        for (int i = 0; i < n_seq; ++i) {
            const int4 s4{seqs[4 * i], seqs[4 * i + 1], seqs[4 * i + 2], seqs[4 * i + 3]};
            if (s4.w < 0 || s4.w >= c.max_batch || seen[s4.w]) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_attn: bad or repeated slot");
            seen[s4.w] = 1;
            if (s4.x != S || s4.y < 1 || s4.z < 0 || s4.z + s4.y >= c.max_seq_len)
                return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_attn: rows not back to back, an empty prompt or one past max_seq_len");
            sq.push_back(s4);
            for (int t = 0; t < s4.y; ++t) rows.push_back(int2{s4.w, s4.z + t});
            S += s4.y;
            max_lp = std::max(max_lp, s4.y);
        }
        if (S > c.max_seq_len) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pf_attn: more rows than a pass holds (max_seq_len)");
    }
    const int HD = c.n_head * c.head_dim;
    const size_t qkvN = (size_t)(c.n_head + 2 * c.n_local_heads) * c.head_dim;
    const size_t cel = (size_t)c.max_batch * ctx->cache_m_stride;
    // NaN patterns in every cache row at or behind a sequence's end and in every slot no sequence names: the kernels must
    // mask or clamp them away by construction
    std::vector<int> end(c.max_batch, 0);
    for (const int4& s4 : sq) end[s4.w] = s4.z + s4.y;
    for (int m = 0; m < c.max_batch; ++m)
        for (int h = 0; h < c.n_local_heads; ++h) {
            const size_t r0 = (size_t)m * ctx->cache_m_stride + ((size_t)h * ctx->n_slots + end[m]) * c.head_dim;
            const size_t n = (size_t)(ctx->n_slots - end[m]) * c.head_dim;
            std::fill(kc + r0, kc + r0 + n, WT_POISON);
            std::fill(vc + r0, vc + r0 + n, WT_POISON);
        }
    DevTmp tmp;
    const std::vector<uint16_t> fill((size_t)(S + 1) * HD, WT_POISON);
    const std::vector<uint32_t> fill32((size_t)(S + 1) * HD, WT_POISON_F32);
    void* dQkv = tmp.put(qkv, (size_t)S * qkvN * sizeof(float));
    void* dQn = tmp.put(qn, (size_t)c.head_dim * 2);
    void* dKn = tmp.put(kn, (size_t)c.head_dim * 2);
    void* dK = tmp.put(kc, cel * 2);
    void* dV = tmp.put(vc, cel * 2);
    void* dY = tmp.put(fill.data(), fill.size() * 2);
    void* dYf = tmp.put(fill32.data(), fill32.size() * 4);
    void* dQ = tmp.put(fill.data(), fill.size() * 2);
    void* dSeq = tmp.put(sq.data(), sq.size() * sizeof(int4));
    void* dRows = n_seq ? tmp.put(rows.data(), rows.size() * sizeof(int2)) : nullptr;
    if (!dQkv || !dQn || !dKn || !dK || !dV || !dY || !dYf || !dQ || !dSeq || (n_seq && !dRows)) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_pf_attn: device temporaries");
    }
    Launch L{ctx, ctx->stream, 0, 1, 0};
    const PfAttnIO io{(const float*)dQkv, dQn, dKn, dK, dV, (float*)dYf, (bf16_t*)dY, (bf16_t*)dQ, (const int4*)dSeq, (const int2*)dRows};
    const RaggedPf rg{n_seq, max_lp};
    *path = n_seq ? pf_attn(L, io, 0, S, 0, &rg) : pf_attn(L, io, slot, Lp, pos0, nullptr);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (L.err != hipSuccess || e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_pf_attn launch failed");
    FT_HIP(ctx, hipMemcpy(y, dY, (size_t)S * HD * 2, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(q, dQ, (size_t)S * HD * 2, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(tail, (const uint16_t*)dY + (size_t)S * HD, (size_t)HD * 2, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(tail + HD, (const uint16_t*)dQ + (size_t)S * HD, (size_t)HD * 2, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(kc, dK, cel * 2, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(vc, dV, cel * 2, hipMemcpyDeviceToHost));
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ decode-launch test hooks (1..max_batch rows)
// (include/fishtts_hip_test.h: ft_test_gemv, ft_test_decode_attn, ft_test_embed).  Host code around gemv, decode_attn_wo and
// the embedding launch on temporaries: nothing here is reached from a frame.
template <typename WT, int ROUND>
static ft_status test_gemv_t(ft_ctx* ctx, int pro, int epi, int M, int N, int K, const float* x, int ldx, const void* W,
                             const void* gain, const void* bias, const float* resid, bool alias, int nt, int ldo, float* out,
                             int32_t* id3) {
    const size_t esz = sizeof(WT);
    std::vector<uint32_t> xh((size_t)((M + 3) / 4 * 4) * ldx, WT_POISON_F32);   // rows M .. 4 ceil(M / 4) - 1 and the ldx padding: NaN patterns
    for (int m = 0; m < M; ++m) memcpy(xh.data() + (size_t)m * ldx, x + (size_t)m * K, (size_t)K * 4);
    std::vector<uint32_t> oh((size_t)(M + 1) * ldo, WT_POISON_F32);   // padding columns and the row behind row M - 1: the sentinel
    std::vector<uint32_t> rh = oh;
    if (epi == EPI_RESID)
        for (int m = 0; m < M; ++m) memcpy(rh.data() + (size_t)m * ldo, resid + (size_t)m * N, (size_t)N * 4);
    DevTmp tmp;
    void* dX = tmp.put(xh.data(), xh.size() * 4);
    void* dW = tmp.put(W, (size_t)N * K * esz);
    void* dG = pro == PRO_RMSNORM ? tmp.put(gain, (size_t)K * esz) : nullptr;
    void* dB = bias ? tmp.put(bias, (size_t)N * esz) : nullptr;
    void* dR = epi == EPI_RESID ? tmp.put(rh.data(), rh.size() * 4) : nullptr;
    void* dO = epi == EPI_RESID && alias ? dR : tmp.put(oh.data(), oh.size() * 4);
    if (!dX || !dW || (pro == PRO_RMSNORM && !dG) || (bias && !dB) || (epi == EPI_RESID && !dR) || !dO) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_gemv: device temporaries");
    }
    Launch L{ctx, ctx->stream, 0, M, 0};
    GemvP p{};
    p.W = dW; p.bias = dB; p.x = (const float*)dX; p.ldx = ldx; p.gain = dG; p.eps = ctx->c.norm_eps;
    p.out = (float*)dO; p.ldo = ldo; p.resid = (const float*)dR; p.ldr = ldo; p.N = N; p.K = K; p.pro = pro; p.epi = epi; p.nt = nt;
    const GemvId id = gemv<WT, ROUND>(L, p, rows_per_wave(N, M));
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (L.err != hipSuccess || e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_gemv launch failed");
    FT_HIP(ctx, hipMemcpy(out, dO, oh.size() * 4, hipMemcpyDeviceToHost));
    id3[0] = id.MB; id3[1] = id.R; id3[2] = id.NT;
    return FT_OK;
}

extern "C" ft_status ft_test_gemv(ft_ctx* ctx, int32_t pro, int32_t epi, int32_t M, int32_t N, int32_t K, const float* x,
                                  int32_t ldx, const void* W, const void* gain, const void* bias, const float* resid,
                                  int32_t alias, int32_t nt, int32_t ldo, float* out, int32_t* id) {
    FT_TRY(ar_ready(ctx));
    const int vec = ctx->c.dtype == FT_F32 ? 4 : 8;
    if (pro != PRO_NONE && pro != PRO_RMSNORM) return ft_fail(ctx, FT_ERR_ARG, "ft_test_gemv: bad prologue");
    if (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU) return ft_fail(ctx, FT_ERR_ARG, "ft_test_gemv: bad epilogue");
    if (M < 1 || M > ctx->c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_test_gemv: M outside 1..max_batch");
    if (K < 8 || K % 8 != 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_gemv: K is not a whole number of 16-byte pieces");
    if (pick_nt(K, vec) < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_gemv: K above 12 x 64 pieces per row");
    if (N < 1 || (epi == EPI_SWIGLU && N % 2 != 0)) return ft_fail(ctx, FT_ERR_ARG, "ft_test_gemv: bad N");
    const int oc = epi == EPI_SWIGLU ? N / 2 : N;
    if (ldx < K || ldx % 4 != 0 || ldo < oc || ldo % 4 != 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_gemv: bad ldx or ldo");
    if (!x || !W || !out || !id || (pro == PRO_RMSNORM && !gain) || (epi == EPI_RESID && !resid))
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_gemv: missing argument");
    return by_dtype(ctx, [&](auto t) { using T = decltype(t); return test_gemv_t<typename T::WT, T::ROUND>(ctx, pro, epi, M, N, K, x, ldx, W, gain, bias, resid, alias != 0, nt != 0, ldo, out, id); });
}

template <typename WT, int ROUND>
static ft_status test_decode_attn_t(ft_ctx* ctx, int M, const float* qkv, const int32_t* pos, int pos_off, const void* qn,
                                    const void* kn, void* kc, void* vc, const void* wo, const void* bo, const float* resid,
                                    float* y, float* part_o, float* part_ml, float* x_out) {
    const ft_ar_config& c = ctx->c;
    const size_t esz = sizeof(WT);
    const int HD = c.n_head * c.head_dim, D = c.dim, ns = ctx->nsplit;
    const size_t qkvN = (size_t)(c.n_head + 2 * c.n_local_heads) * c.head_dim;
    const size_t cbytes = (size_t)M * ctx->cache_m_stride * esz;
    const size_t n_po = (size_t)M * c.n_head * ns * c.head_dim, n_pm = (size_t)M * c.n_head * ns * 2;
    const std::vector<uint32_t> yfill((size_t)M * ctx->y_ld, WT_POISON_F32);
    DevTmp tmp;
    void* dQ = tmp.put(qkv, (size_t)M * qkvN * sizeof(float));
    void* dP = tmp.put(pos, (size_t)M * sizeof(int));
    void* dQn = qn ? tmp.put(qn, (size_t)c.head_dim * esz) : nullptr;
    void* dKn = kn ? tmp.put(kn, (size_t)c.head_dim * esz) : nullptr;
    void* dK = tmp.put(kc, cbytes);
    void* dV = tmp.put(vc, cbytes);
    void* dW = tmp.put(wo, (size_t)D * HD * esz);
    void* dB = bo ? tmp.put(bo, (size_t)D * esz) : nullptr;
    void* dX = tmp.put(resid, (size_t)M * D * sizeof(float));
    void* dY = tmp.put(yfill.data(), yfill.size() * 4);
    if (!dQ || !dP || (qn && !dQn) || (kn && !dKn) || !dK || !dV || !dW || (bo && !dB) || !dX || !dY) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_decode_attn: device temporaries");
    }
    if (ns > 1) {   // the context's split-partial scratch: every (O, m, l) of this call must be written by the launch
        const std::vector<uint32_t> pf(n_po, WT_POISON_F32);
        FT_HIP(ctx, hipMemcpy(ctx->part_o, pf.data(), n_po * 4, hipMemcpyHostToDevice));
        FT_HIP(ctx, hipMemcpy(ctx->part_ml, pf.data(), n_pm * 4, hipMemcpyHostToDevice));
    }
    Launch L{ctx, ctx->stream, 0, M, pos_off};
    AttnP a{};
    a.qkv = (const float*)dQ; a.ldq = (int)qkvN; a.qn = dQn; a.kn = dKn; a.rope = ctx->rope;
    a.kc = dK; a.vc = dV; a.cache_m_stride = ctx->cache_m_stride; a.pos = (const int*)dP; a.pos_off = pos_off;
    a.H = c.n_head; a.Hkv = c.n_local_heads; a.hd = c.head_dim; a.n_slots = ctx->n_slots;
    a.nsplit = ns; a.eps = c.norm_eps; a.scale = 1.0f / sqrtf((float)c.head_dim);
    a.y = (float*)dY; a.ldy = ctx->y_ld;
    a.part_o = ctx->part_o; a.part_ml = ctx->part_ml;
    GemvP o{};
    o.W = dW; o.bias = dB; o.x = (const float*)dY; o.ldx = ctx->y_ld; o.out = (float*)dX; o.ldo = D;
    o.resid = (const float*)dX; o.ldr = D; o.N = D; o.K = HD; o.pro = PRO_NONE; o.epi = EPI_RESID; o.nt = 1;
    decode_attn_wo<WT, ROUND>(L, a, o);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (L.err != hipSuccess || e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_decode_attn launch failed");
    FT_HIP(ctx, hipMemcpy(y, dY, yfill.size() * 4, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(x_out, dX, (size_t)M * D * 4, hipMemcpyDeviceToHost));
    if (ns > 1) {
        FT_HIP(ctx, hipMemcpy(part_o, ctx->part_o, n_po * 4, hipMemcpyDeviceToHost));
        FT_HIP(ctx, hipMemcpy(part_ml, ctx->part_ml, n_pm * 4, hipMemcpyDeviceToHost));
    }
    FT_HIP(ctx, hipMemcpy(kc, dK, cbytes, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(vc, dV, cbytes, hipMemcpyDeviceToHost));
    return FT_OK;
}

extern "C" ft_status ft_test_decode_attn(ft_ctx* ctx, int32_t M, const float* qkv, const int32_t* pos, int32_t pos_off,
                                         const void* qn, const void* kn, void* kc, void* vc, const void* wo, const void* bo,
                                         const float* resid, int32_t* nsplit, float* y, float* part_o, float* part_ml,
                                         float* x_out) {
    FT_TRY(ar_ready(ctx));
    if (M < 1 || M > ctx->c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_test_decode_attn: M outside 1..max_batch");
    if (!qkv || !pos || !kc || !vc || !wo || !resid || !nsplit || !y || !part_o || !part_ml || !x_out)
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_decode_attn: missing argument");
    if (pos_off < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_decode_attn: negative pos_off");
    int pos_end = 0;
    for (int m = 0; m < M; ++m) {
        if (pos[m] < 0 || pos[m] + pos_off >= ctx->n_slots || pos[m] + pos_off >= ctx->c.max_seq_len)
            return ft_fail(ctx, FT_ERR_ARG, "ft_test_decode_attn: a position outside the cache or the rope table");
        pos_end = std::max(pos_end, pos[m] + pos_off + 1);
    }
    const int saved = ctx->nsplit;
    pick_nsplit(ctx, pos_end);       // as ft_ar_decode does for the longest context of its call
    *nsplit = ctx->nsplit;
    const ft_status st = by_dtype(ctx, [&](auto t) { using T = decltype(t); return test_decode_attn_t<typename T::WT, T::ROUND>(ctx, M, qkv, pos, pos_off, qn, kn, kc, vc, wo, bo, resid, y, part_o, part_ml, x_out); });
    ctx->nsplit = saved;
    return st;
}

template <typename WT, int ROUND>
static ft_status test_embed_t(ft_ctx* ctx, int M, int D, int ncb, int cbsize, int vocab, const void* emb, const void* cb_emb,
                              const int32_t* toks, int64_t n_toks, int64_t trs, int64_t tms, int sem_begin, int sem_end, int scale,
                              int ldx, int xo_ldm, float* x, uint16_t* xo) {
    const size_t esz = sizeof(WT);
    const std::vector<uint32_t> xfill((size_t)(M + 1) * ldx, WT_POISON_F32);
    const size_t n_xo = (size_t)((D + 7) / 8) * xo_ldm * 8;
    const std::vector<uint16_t> ofill(n_xo, WT_POISON);
    DevTmp tmp;
    void* dE = tmp.put(emb, (size_t)vocab * D * esz);
    void* dC = tmp.put(cb_emb, (size_t)ncb * cbsize * D * esz);
    void* dT = tmp.put(toks, (size_t)n_toks * sizeof(int));
    void* dX = tmp.put(xfill.data(), xfill.size() * 4);
    void* dO = xo_ldm > 0 ? tmp.put(ofill.data(), n_xo * 2) : nullptr;
    if (!dE || !dC || !dT || !dX || (xo_ldm > 0 && !dO)) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_embed: device temporaries");
    }
    EmbedP e{};
    e.emb = dE; e.cb_emb = dC; e.toks = (const int*)dT; e.tok_row_stride = (long)trs; e.tok_m_stride = (long)tms; e.col = 0;
    e.x = (float*)dX; e.ldx = ldx; e.D = D; e.ncb = ncb; e.cbsize = cbsize; e.vocab = vocab; e.sem_begin = sem_begin;
    e.sem_end = sem_end; e.scale = scale; e.inv_div = (float)sqrt((double)(ncb + 1));
    e.xo = (bf16_t*)dO; e.xo_ldm = xo_ldm;
    embed_kernel<WT, ROUND><<<dim3((D + 255) / 256, M), 256, 0, ctx->stream>>>(e);
    const hipError_t le = hipGetLastError(), se = hipStreamSynchronize(ctx->stream);
    if (le != hipSuccess || se != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_embed launch failed");
    FT_HIP(ctx, hipMemcpy(x, dX, xfill.size() * 4, hipMemcpyDeviceToHost));
    if (xo_ldm > 0) FT_HIP(ctx, hipMemcpy(xo, dO, n_xo * 2, hipMemcpyDeviceToHost));
    return FT_OK;
}

extern "C" ft_status ft_test_embed(ft_ctx* ctx, int32_t M, int32_t D, int32_t ncb, int32_t cbsize, int32_t vocab, const void* emb,
                                   const void* cb_emb, const int32_t* toks, int64_t n_toks, int64_t tok_row_stride,
                                   int64_t tok_m_stride, int32_t sem_begin, int32_t sem_end, int32_t scale, int32_t ldx,
                                   int32_t xo_ldm, float* x, uint16_t* xo) {
    FT_TRY(ar_ready(ctx));
    if (M < 1 || M > 65535 || D < 1 || ncb < 1 || cbsize < 1 || vocab < 1 || ldx < D)
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_embed: bad size");
    if (!emb || !cb_emb || !toks || !x || (xo_ldm > 0 && !xo)) return ft_fail(ctx, FT_ERR_ARG, "ft_test_embed: missing argument");
    if (xo_ldm < 0 || (xo_ldm > 0 && (ctx->c.dtype == FT_F32 || M > xo_ldm)))
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_embed: the octet-major copy is 16-bit, of at most xo_ldm rows");
    if (tok_row_stride < 0 || tok_m_stride < 0 || (int64_t)(M - 1) * tok_m_stride + (int64_t)ncb * tok_row_stride >= n_toks)
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_embed: the token strides reach past toks");
    return by_dtype(ctx, [&](auto t) { using T = decltype(t); return test_embed_t<typename T::WT, T::ROUND>(ctx, M, D, ncb, cbsize, vocab, emb, cb_emb, toks, n_toks,
                                                                      tok_row_stride, tok_m_stride, sem_begin, sem_end, scale, ldx, xo_ldm, x, xo); });
}

template <typename WT, int ROUND>
static ft_status test_fast_attn_t(ft_ctx* ctx, int form, int M, int cpos, const float* qkv, const void* qn, const void* kn, void* kc,
                                  void* vc, float* y, uint16_t* y_bf) {
    const ft_ar_config& c = ctx->c;
    const size_t esz = sizeof(WT);
    const int Hf = c.fast_n_head, Hkvf = c.fast_n_local_heads, hdf = c.fast_head_dim, HDf = Hf * hdf, ncb = c.num_codebooks;
    const size_t qkvN = (size_t)(Hf + 2 * Hkvf) * hdf;
    const int rows = form == 2 ? ctx->xo_pair + M : M;
    const size_t cel = (size_t)M * ctx->fcache_m_stride;
    // NaN patterns in every cache row the launch appends or must not read: from c on (the paired pass: from row 0 on)
    const int first = form == 2 ? 0 : cpos;
    for (int m = 0; m < M; ++m)
        for (int h = 0; h < Hkvf; ++h) {
            char* k0 = (char*)kc + ((size_t)m * ctx->fcache_m_stride + ((size_t)h * ncb + first) * hdf) * esz;
            char* v0 = (char*)vc + ((size_t)m * ctx->fcache_m_stride + ((size_t)h * ncb + first) * hdf) * esz;
            memset(k0, 0xFF, (size_t)(ncb - first) * hdf * esz);          // all-ones: a NaN in bf16, fp16 and f32
            memset(v0, 0xFF, (size_t)(ncb - first) * hdf * esz);
        }
    std::vector<uint32_t> qh((size_t)rows * qkvN, WT_POISON_F32);        // paired: rows M .. xo_pair - 1 belong to nobody
    memcpy(qh.data(), qkv, (size_t)M * qkvN * 4);
    if (form == 2) memcpy(qh.data() + (size_t)ctx->xo_pair * qkvN, qkv + (size_t)M * qkvN, (size_t)M * qkvN * 4);
    const int ldm = ctx->xo_ldm;
    const std::vector<uint32_t> yfill((size_t)(M + 1) * ctx->y_ld, WT_POISON_F32);
    const std::vector<uint16_t> bfill(form ? (size_t)HDf * ldm : 0, WT_POISON);
    DevTmp tmp;
    void* dQ = tmp.put(qh.data(), qh.size() * 4);
    void* dQn = qn ? tmp.put(qn, (size_t)hdf * esz) : nullptr;
    void* dKn = kn ? tmp.put(kn, (size_t)hdf * esz) : nullptr;
    void* dK = tmp.put(kc, cel * esz);
    void* dV = tmp.put(vc, cel * esz);
    void* dY = form == 0 ? tmp.put(yfill.data(), yfill.size() * 4) : tmp.put(bfill.data(), bfill.size() * 2);
    if (!dQ || (qn && !dQn) || (kn && !dKn) || !dK || !dV || !dY) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_test_fast_attn: device temporaries");
    }
    FastAttnP a{};
    a.qkv = (const float*)dQ; a.ldq = (int)qkvN; a.qn = dQn; a.kn = dKn; a.rope = ctx->frope;
    a.kc = dK; a.vc = dV; a.cache_m_stride = ctx->fcache_m_stride; a.c = form == 2 ? 0 : cpos; a.H = Hf; a.Hkv = Hkvf; a.hd = hdf;
    a.ncb = ncb; a.eps = c.norm_eps; a.scale = (float)(1.0 / sqrt((double)hdf));
    if (form == 0) {
        fast_attn_kernel<WT, ROUND><<<dim3(Hf, M), 64, 0, ctx->stream>>>(a, (float*)dY, ctx->y_ld);
    } else {
        a.y_bf = (bf16_t*)dY; a.y_xo_ldm = ldm;
        a.pair_M = form == 2 ? M : 0; a.pair_off = ctx->xo_pair;
        fast_attn_kernel<WT, ROUND><<<dim3(Hf, form == 2 ? 2 * M : M), 64, 0, ctx->stream>>>(a, nullptr, HDf);
    }
    const hipError_t le = hipGetLastError(), se = hipStreamSynchronize(ctx->stream);
    if (le != hipSuccess || se != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, "ft_test_fast_attn launch failed");
    if (form == 0) FT_HIP(ctx, hipMemcpy(y, dY, yfill.size() * 4, hipMemcpyDeviceToHost));
    else FT_HIP(ctx, hipMemcpy(y_bf, dY, bfill.size() * 2, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(kc, dK, cel * esz, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipMemcpy(vc, dV, cel * esz, hipMemcpyDeviceToHost));
    return FT_OK;
}

extern "C" ft_status ft_test_fast_attn(ft_ctx* ctx, int32_t form, int32_t M, int32_t cpos, const float* qkv, const void* qn,
                                       const void* kn, void* kc, void* vc, float* y, uint16_t* y_bf) {
    FT_TRY(ar_ready(ctx));
    const ft_ar_config& c = ctx->c;
    if (form < 0 || form > 2) return ft_fail(ctx, FT_ERR_ARG, "ft_test_fast_attn: bad form");
    if (!qkv || !kc || !vc || (form == 0 ? !y : !y_bf)) return ft_fail(ctx, FT_ERR_ARG, "ft_test_fast_attn: missing argument");
    if (c.n_fast_layer < 1 || c.num_codebooks > FAST_MAXCB || c.fast_head_dim > 128)
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_fast_attn: this context has no fast stack the kernel takes");
    if (form == 0) {
        if (M < 1 || M > c.max_batch) return ft_fail(ctx, FT_ERR_ARG, "ft_test_fast_attn: M outside 1..max_batch");
    } else {
        if (c.dtype == FT_F32) return ft_fail(ctx, FT_ERR_ARG, "ft_test_fast_attn: the wide forms are 16-bit");
        if (!ctx->wide_ok) return ft_fail(ctx, FT_ERR_STATE, "ft_test_fast_attn: this context has no lock-step MFMA path");
        if (M < 5 || M > 64 || M > ctx->xo_ldm) return ft_fail(ctx, FT_ERR_ARG, "ft_test_fast_attn: M outside 5..min(64, xo_ldm)");
        // The hook is wider than the product's rule on purpose.  wide_pair pairs where xo_pair + M <= 64; the hook also takes
        // every M that fits the buffers of a context of up to 64 rows (xo_pair <= 64, M <= xo_ldm - xo_pair), so that the kernel's
        // paired form is checked at every tile edge up to 64 rows on the one 64-row context the kernel tests share, not only
        // at the M a context's own xo_pair admits.  Above 64 rows (xo_pair >= 80) no M pairs in the product and none is added
        // by a larger context: refused.
        if (form == 2 && (c.num_codebooks < 2 || ctx->xo_pair > 64 || ctx->xo_pair + M > ctx->xo_ldm))
            return ft_fail(ctx, FT_ERR_ARG, "ft_test_fast_attn: the paired pass does not fit");
    }
    if (form != 2 && (cpos < 0 || cpos >= c.num_codebooks)) return ft_fail(ctx, FT_ERR_ARG, "ft_test_fast_attn: c outside 0..ncb-1");
    return by_dtype(ctx, [&](auto t) { using T = decltype(t); return test_fast_attn_t<typename T::WT, T::ROUND>(ctx, form, M, cpos, qkv, qn, kn, kc, vc, y, y_bf); });
}
