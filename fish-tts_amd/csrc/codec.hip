// DAC codec decode (DAC.decode, vocoder.py:906-912) on the tap-GEMM kernels of gemm_kernels.h.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <numeric>

#include "codec_kernels.h"
#include "stage_kernels.h"
#include "stereo_kernels.h"
#include "room_kernels.h"
#include "flac_kernels.h"
#include "engine.h"
#include "fx_chain.h"
#include "join_plan.h"
#include "item_fx.h"

using namespace ft;
// the output chain's host arithmetic (fx_chain.h), on the kernels' constants
using chain::ChainPlan; using chain::FxDesc; using chain::StageChain; using chain::StagePlan;
using chain::RS_FI; using chain::RS_MAX_RATE;
static_assert(chain::RS_LDS == RS_LDS && chain::TS_N == TS_N && chain::TS_HS == TS_HS && chain::TS_D == TS_D &&
              chain::TS_CARRY == TS_CARRY && chain::PS_SHIFT == PS_SHIFT && chain::PS_PHASES == PS_PHASES &&
              chain::LV_WARM_HOPS == LV_WARM && chain::RD_A == RD_LOOK && chain::RD_R == RD_SLEW &&
              chain::MX_MAX_W == MX_MAX_WIN && chain::MX_MAX_N <= (1LL << 28),
              "fx_chain.h and stage_kernels.h disagree");
static_assert(sizeof(ft_level_info) == 32 && offsetof(LevelItem, L) + sizeof(ft_level_info) == sizeof(LevelItem) &&
              offsetof(ft_level_info, peak) == 8 && offsetof(ft_level_info, capped) == 24 &&
              offsetof(LevelItem, target) == offsetof(LevelItem, L) + 28,
              "ft_level_info is the tail of a LevelItem, the item's target in the bytes that pad it");

#define FT_TRY(x) do { ft_status s_ = (x); if (s_ != FT_OK) return s_; } while (0)

struct ConvW {            // one packed tap-GEMM weight
    bf16_t* w = nullptr;  // [ntap][N][K]
    float* bias = nullptr;
    int ntap = 1, N = 0, K = 0, n_mod = 0;
    int offs[8] = {0};
};
struct TfLayer { ConvW qkv, wo, w13, w2; float *n1, *n2, *g1, *g2; };
struct UpStage { ConvW ct; float *dw_w, *dw_b, *ln_w, *ln_b, *gamma; ConvW pw1, pw2; int f; };
struct ResUnitW { float *a0, *a2; ConvW c7, c1; };
struct DecBlock { float* a0; ConvW ct; ResUnitW u[3]; int s, cin, cout; };

struct ft_codec_stream;
struct ft_mix_stream;
struct ft_room_stream;
struct ft_flac_stream;
struct CodecState {
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::vector<ft_codec_stream*> streams;   // live streamed decodes of this context (their device state is freed with it)
    float* tables = nullptr;  // RVQ tables
    float* rope = nullptr;
    std::vector<TfLayer> tf;
    float* tf_norm = nullptr;
    std::vector<UpStage> up;
    ConvW conv_in;
    std::vector<DecBlock> blocks;
    float* a_last = nullptr;
    float* w_last = nullptr;  // [7][C]
    float b_last = 0.f;
    int c_last = 0;
    std::vector<void*> owned;
    // activations (one batch item at a time)
    int* codes = nullptr;
    float *x = nullptr, *audio = nullptr;
    bf16_t *xn = nullptr, *qkv = nullptr, *y = nullptr, *g = nullptr;
    bf16_t* big[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t big_elems = 0, big_margin = 0;
    int frame_len = 0, up_total = 1;
    // batched streamed decode (ft_codec_stream_decode_many): its own conv buffers and q k v work buffer (a carried-row
    // margin in front of every chunk) and a device table of chunks, carries and codes; allocated on its first call
    bf16_t* mbig[4] = {nullptr, nullptr, nullptr, nullptr};
    bf16_t* mqkv = nullptr;
    unsigned char* mtab = nullptr;
    int mcarry = 0;           // carries per stream (convolution tails + one K/V per transformer layer)
    // resampler (ft_codec_decode_at, ft_codec_stream_*_at): one [L][K] table per output rate, uploaded on its first use;
    // an output buffer and a segment table, allocated on the first resampled call
    using RsTab = chain::RsTab;
    std::map<int, RsTab> rs_tabs;
    float* rs_out = nullptr;
    size_t rs_cap = 0;
    RsSeg* rs_seg = nullptr;
    // time-scale stage (ft_codec_decode_fx, ft_codec_stream_begin_fx): the window, an output buffer (the resampler's input
    // then), a segment table and the test hook's d_k, allocated on the first time-scaled call
    float *ts_win = nullptr, *ts_out = nullptr;
    size_t ts_cap = 0;
    TsSeg* ts_seg = nullptr;
    int* ts_delta = nullptr;
    // pitch stage (ft_codec_decode_fxp, ft_codec_stream_begin_fxp): one [513][K] table per cents value, uploaded on its first
    // use; an output buffer (the resampler's input then) and a segment table, allocated on the first pitched call
    using PsTab = chain::PsTab;
    std::map<int, PsTab> ps_tabs;
    float* ps_out = nullptr;
    PsSeg* ps_seg = nullptr;
    // join stage (ft_codec_decode_join): the items of a call side by side at the output rate, the joined waveform and the
    // item table, allocated on the first joined call (the two buffers grow when a later call needs more)
    float *join_in = nullptr, *join_out = nullptr;
    size_t join_in_cap = 0, join_out_cap = 0;
    JoinTab* join_tab = nullptr;
    // level stage (ft_codec_loudness, ft_codec_decode_level, ft_codec_decode_join_level): the item table, one hop sum and
    // one hop peak per 100 ms of a call's items, the host copies of the table on its way there and back, and the waveform
    // of ft_codec_loudness; allocated on the first levelled call (the buffers grow when a later call needs more)
    // reference intake (ft_codec_intake, ft_codec_encode_items): one [L][K] table per input rate, uploaded on its first use; the
    // raw bytes of a call's clips (every clip on a 16-byte boundary), the segment table with the counters behind it, and the
    // codes of a call's clips gathered for one copy; allocated on the first intake call (the buffers grow on need)
    std::map<int, RsTab> in_tabs;
    unsigned char* in_raw = nullptr;
    size_t in_raw_cap = 0;
    IntakeSeg* in_seg = nullptr;
    unsigned long long* in_count = nullptr;
    int* in_codes = nullptr;
    size_t in_codes_cap = 0;
    // mix stage (ft_codec_mix): the gain table, uploaded once; the programme, the bed at the output rate, the output, the
    // activity flags, D_k and g_k, and the three words the launches reduce into; allocated on the first mixed call (the
    // buffers grow on need)
    float *mx_T = nullptr, *mx_x = nullptr, *mx_bed = nullptr, *mx_y = nullptr, *mx_g = nullptr;
    unsigned char* mx_act = nullptr;
    int* mx_D = nullptr;
    MixOut* mx_out = nullptr;
    size_t mx_xcap = 0, mx_bedcap = 0, mx_ycap = 0, mx_gcap = 0, mx_actcap = 0, mx_Dcap = 0;
    // stereo mix stage (ft_codec_mix_stereo): the pan table, uploaded once, and the call's regions; the rest is the mix
    // stage's (mx_bed then holds both sides, mx_y the 2 N interleaved floats)
    float* mx_U = nullptr;
    MixPan* mx_reg = nullptr;
    size_t mx_regcap = 0;
    // room stage (ft_codec_room): the sent programme, t and hn, the block energies, the words the launches reduce into; the
    // programme, the output and the regions use the mix stage's buffers (the stages never run inside one call)
    float *rm_xs = nullptr, *rm_t = nullptr, *rm_hn = nullptr;
    double* rm_e = nullptr;
    RoomOut* rm_out = nullptr;
    size_t rm_xscap = 0, rm_tcap = 0, rm_hncap = 0, rm_ecap = 0;
    // FLAC stage (ft_codec_flac): the raw samples, one decision per frame and signal, the frames at their worst-case stride,
    // their lengths and places, the compact stream, the counters; allocated on the first call (the buffers grow on need)
    unsigned char *fl_in = nullptr, *fl_slots = nullptr, *fl_stream = nullptr;
    FlSig* fl_sig = nullptr;
    int* fl_len = nullptr;
    long long* fl_off = nullptr;
    FlacOut* fl_out = nullptr;
    size_t fl_incap = 0, fl_slotcap = 0, fl_streamcap = 0, fl_sigcap = 0, fl_lencap = 0, fl_offcap = 0;
    // live FLAC stage (ft_codec_flac_stream_*): the open streams, as mix_streams, and the int16 staging buffer of a push
    // (carry || push, quantised); a push's raw samples lie in fl_in, its frames in the FLAC stage's buffers
    std::vector<ft_flac_stream*> flac_streams;
    short* fl_stage = nullptr;
    size_t fl_stagecap = 0;
    // live mix stage (ft_codec_mix_stream_*): the open streams (their device state is freed with the context), and what a
    // push stages - its samples, the m of the hops it completes, the samples it emits; the buffers grow on need
    std::vector<ft_mix_stream*> mix_streams;
    std::vector<ft_room_stream*> room_streams;   // live room stage (ft_codec_room_stream_*): the open streams, as mix_streams
    float *ml_x = nullptr, *ml_m = nullptr, *ml_y = nullptr;
    size_t ml_xcap = 0, ml_mcap = 0, ml_ycap = 0;
    unsigned char* ml_q = nullptr;    // live stereo mix stage: the pan bytes of a push
    size_t ml_qcap = 0;
    LevelTab* lv_tab = nullptr;
    double* lv_hops = nullptr;
    float *lv_peaks = nullptr, *lv_x = nullptr;
    size_t lv_cap = 0, lv_xcap = 0, lv_nhops = 0;
    std::vector<char> lv_up, lv_down;
    // ride stage (ft_codec_stream_begin_live, ft_codec_ride): the segment table and the buffer the emitted samples of a call
    // lie in back to back, allocated with the first live stream; the state of ft_codec_ride's one waveform (hop sums, v,
    // peaks, nodes), which grows like the level stage's buffers
    RdSeg* rd_seg = nullptr;
    float* rd_out = nullptr;
    size_t rd_cap = 0;
    double *rd_e = nullptr, *rd_v = nullptr;
    float *rd_p = nullptr, *rd_g = nullptr;
    size_t rd_ecap = 0, rd_vcap = 0, rd_pcap = 0, rd_gcap = 0;
    // ---- encode side
    struct EncUnit { float *a0, *a2; ConvW c7, c1; };
    struct EncBlock { EncUnit u[3]; float* a3; ConvW sc; int s, cin, cout; std::vector<TfLayer> tf; float* tf_norm = nullptr; };
    bool has_enc = false;
    float *enc_w0 = nullptr, *enc_b0 = nullptr;   // first conv [C][7], [C]
    std::vector<EncBlock> enc;
    float* enc_a_last = nullptr;
    ConvW enc_out;                                 // k = 3 conv to the latent
    std::vector<UpStage> down;                     // quantizer.downsample (ct = strided conv here)
    std::vector<TfLayer> pre;
    float* pre_norm = nullptr;
    float *rope_enc = nullptr, *inw = nullptr, *inb = nullptr, *cbn = nullptr, *cn2 = nullptr;
    float *enc_audio = nullptr, *enc_x = nullptr, *enc_zq = nullptr;
    bf16_t *ebuf[4] = {nullptr, nullptr, nullptr, nullptr}, *e_xn = nullptr, *e_qkv = nullptr, *e_y = nullptr, *e_g = nullptr;
    int* enc_codes = nullptr;
    int hop = 1, enc_frame_len = 0;
    long max_samples = 0;
    // ---- test hook (fishtts_hip_test.h, ft_test_codec_trace_*): `trace` is non-null only inside a traced one-shot
    // decode / encode or a traced streamed decode; every launch site tests it once
    struct TraceBuf { int kind = 0, f32 = 0; long elems = 0; std::vector<char> data; };   // kind: 0 out_bf, 1 out_act, 2 out_f32
    struct TraceRec { std::string name; int rows = 0, cols = 0, variant = -1, halo = 0, ntap = 0, K = 0; bool held = false; std::vector<TraceBuf> bufs; };
    struct TraceChunk { int P, L, t0, nh; };
    struct Trace {
        int first = 0, count = 0;
        bool armed = false, failed = false;
        std::vector<TraceRec> recs;
        std::vector<TraceChunk> chunks;   // a streamed call: its chunks {P, L, t0, nh} in call order; empty: a one-shot call
        bool batched = false;             // ft_codec_stream_decode_many: gap rows in front of every chunk
        long frames = 0;                  // frames of all chunks
    };
    Trace tstore;
    Trace* trace = nullptr;
};

static std::string cname(const char* fmt, int a = 0, int b = 0) {
    char buf[160];
    snprintf(buf, sizeof buf, fmt, a, b);
    return buf;
}

// samples one encode call may hold, and the most positions an encoder transformer sees (head_dim 64: 32 rope pairs)
static long enc_max_samples(const ft_codec_config& c) {
    long hop = 1;
    for (int i = 0; i < c.n_enc_rates; ++i) hop *= c.enc_rates[i];
    return (long)c.max_enc_frames * hop * 4;
}
static int64_t enc_rope_positions(const ft_codec_config& c) {
    long rate = 1, best = 1;
    for (int i = 0; i < c.n_enc_rates; ++i) {
        rate *= c.enc_rates[i];
        if (c.enc_tf_layers[i] > 0) best = std::max(best, enc_max_samples(c) / rate);
    }
    return best;
}

void codec_expected(ft_ctx* ctx) {
    const ft_codec_config& c = ctx->cc;
    const int D = c.latent_dim, H = c.tf_n_head * c.tf_head_dim;
    auto E = [&](const std::string& n, std::vector<int64_t> s) { ft_expect(ctx, n, std::move(s), FT_F32); };
    auto tf_layer = [&](const std::string& p, int d, int h, int ffn) {   // one window-transformer layer of width d
        E(p + ".attention.wqkv.weight", {3 * h, d});
        E(p + ".attention.wo.weight", {d, h});
        E(p + ".feed_forward.w1.weight", {ffn, d});
        E(p + ".feed_forward.w3.weight", {ffn, d});
        E(p + ".feed_forward.w2.weight", {d, ffn});
        E(p + ".ffn_norm.weight", {d});
        E(p + ".attention_norm.weight", {d});
        E(p + ".attention_layer_scale.gamma", {d});
        E(p + ".ffn_layer_scale.gamma", {d});
    };
    auto resample_stage = [&](const std::string& p) {   // quantizer.upsample / downsample: (transposed) conv k = s = 2, ConvNeXt
        E(p + ".0.conv.weight", {D, D, 2});
        E(p + ".0.conv.bias", {D});
        E(p + ".1.dwconv.conv.weight", {D, 1, 7});
        E(p + ".1.dwconv.conv.bias", {D});
        E(p + ".1.norm.weight", {D});
        E(p + ".1.norm.bias", {D});
        E(p + ".1.pwconv1.weight", {4 * D, D});
        E(p + ".1.pwconv1.bias", {4 * D});
        E(p + ".1.pwconv2.weight", {D, 4 * D});
        E(p + ".1.pwconv2.bias", {D});
        E(p + ".1.gamma", {D});
    };
    E("quantizer.semantic_quantizer.quantizers.0.codebook.weight", {c.semantic_codebook_size, c.codebook_dim});
    E("quantizer.semantic_quantizer.quantizers.0.out_proj.weight", {D, c.codebook_dim, 1});
    E("quantizer.semantic_quantizer.quantizers.0.out_proj.bias", {D});
    for (int i = 0; i < c.n_codebooks; ++i) {
        E(cname("quantizer.quantizer.quantizers.%d.codebook.weight", i), {c.codebook_size, c.codebook_dim});
        E(cname("quantizer.quantizer.quantizers.%d.out_proj.weight", i), {D, c.codebook_dim, 1});
        E(cname("quantizer.quantizer.quantizers.%d.out_proj.bias", i), {D});
    }
    for (int l = 0; l < c.n_tf_layer; ++l) tf_layer(cname("quantizer.post_module.layers.%d", l), D, H, c.tf_ffn);
    E("quantizer.post_module.norm.weight", {D});
    for (int j = 0; j < c.n_upsample; ++j) resample_stage(cname("quantizer.upsample.%d", j));
    E("decoder.model.0.conv.weight", {c.decoder_dim, D, 7});
    E("decoder.model.0.conv.bias", {c.decoder_dim});
    for (int i = 0; i < c.n_rates; ++i) {
        const int cin = c.decoder_dim >> i, cout = c.decoder_dim >> (i + 1), r = c.rates[i];
        const std::string p = cname("decoder.model.%d.block", i + 1);
        E(p + ".0.alpha", {1, cin, 1});
        E(p + ".1.conv.weight", {cin, cout, 2 * r});
        E(p + ".1.conv.bias", {cout});
        for (int u = 0; u < 3; ++u) {
            const std::string q = p + cname(".%d.block", u + 2);
            E(q + ".0.alpha", {1, cout, 1});
            E(q + ".1.conv.weight", {cout, cout, 7});
            E(q + ".1.conv.bias", {cout});
            E(q + ".2.alpha", {1, cout, 1});
            E(q + ".3.conv.weight", {cout, cout, 1});
            E(q + ".3.conv.bias", {cout});
        }
    }
    const int last = c.decoder_dim >> c.n_rates;
    E(cname("decoder.model.%d.alpha", c.n_rates + 1), {1, last, 1});
    E(cname("decoder.model.%d.conv.weight", c.n_rates + 2), {1, last, 7});
    E(cname("decoder.model.%d.conv.bias", c.n_rates + 2), {1});
    ft_expect(ctx, "rope.codec", {c.max_frames, c.tf_head_dim / 2, 2}, FT_F32);
    if (c.encoder_dim <= 0) return;
    // encode side: Encoder (vocoder.py:539-575), quantizer.downsample / pre_module / in_proj (683-757)
    int d = c.encoder_dim;
    E("encoder.block.0.conv.weight", {d, 1, 7});
    E("encoder.block.0.conv.bias", {d});
    for (int i = 0; i < c.n_enc_rates; ++i) {
        d *= 2;
        const std::string p = cname("encoder.block.%d.block", i + 1);
        for (int u = 0; u < 3; ++u) {
            const std::string q = p + cname(".%d.block", u);
            E(q + ".0.alpha", {1, d / 2, 1});
            E(q + ".1.conv.weight", {d / 2, d / 2, 7});
            E(q + ".1.conv.bias", {d / 2});
            E(q + ".2.alpha", {1, d / 2, 1});
            E(q + ".3.conv.weight", {d / 2, d / 2, 1});
            E(q + ".3.conv.bias", {d / 2});
        }
        E(p + ".3.alpha", {1, d / 2, 1});
        E(p + ".4.conv.weight", {d, d / 2, 2 * c.enc_rates[i]});
        E(p + ".4.conv.bias", {d});
        for (int l = 0; l < c.enc_tf_layers[i]; ++l) tf_layer(p + cname(".5.layers.%d", l), d, d, 3 * d);
        if (c.enc_tf_layers[i]) E(p + ".5.norm.weight", {d});
    }
    E(cname("encoder.block.%d.alpha", c.n_enc_rates + 1), {1, d, 1});
    E(cname("encoder.block.%d.conv.weight", c.n_enc_rates + 2), {D, d, 3});
    E(cname("encoder.block.%d.conv.bias", c.n_enc_rates + 2), {D});
    for (int j = 0; j < c.n_upsample; ++j) resample_stage(cname("quantizer.downsample.%d", j));
    for (int l = 0; l < c.n_tf_layer; ++l) tf_layer(cname("quantizer.pre_module.layers.%d", l), D, H, c.tf_ffn);
    E("quantizer.pre_module.norm.weight", {D});
    E("quantizer.semantic_quantizer.quantizers.0.in_proj.weight", {c.codebook_dim, D, 1});
    E("quantizer.semantic_quantizer.quantizers.0.in_proj.bias", {c.codebook_dim});
    for (int i = 0; i < c.n_codebooks; ++i) {
        E(cname("quantizer.quantizer.quantizers.%d.in_proj.weight", i), {c.codebook_dim, D, 1});
        E(cname("quantizer.quantizer.quantizers.%d.in_proj.bias", i), {c.codebook_dim});
    }
    ft_expect(ctx, "rope.codec_enc", {enc_rope_positions(c), 32, 2}, FT_F32);
}

ft_status codec_create(ft_ctx* ctx) {
    const ft_codec_config& c = ctx->cc;
    auto bad = [&](const char* m) { return ft_fail(ctx, FT_ERR_UNSUPPORTED, m); };
    if (c.dtype != FT_BF16) return bad("codec: only FT_BF16 contractions (f32 accumulate) are implemented");
    if (c.n_upsample < 0 || c.n_upsample > 4 || c.n_rates < 1 || c.n_rates > 8) return bad("codec: bad stage counts");
    if (c.latent_dim % 32 || (c.tf_n_head * c.tf_head_dim) % 32 || c.tf_ffn % 32 || c.decoder_dim % 32)
        return bad("codec: channel counts must be multiples of 32");
    if ((c.decoder_dim >> c.n_rates) % 32) return bad("codec: decoder_dim / 2^n_rates must be a multiple of 32");
    if (c.tf_head_dim > 128 || c.tf_head_dim % 8 || c.tf_window > 512) return bad("codec: head_dim <= 128, window <= 512");
    if (c.encoder_dim > 0) {
        if (c.n_enc_rates < 1 || c.n_enc_rates > 8 || c.encoder_dim % 32 || c.max_enc_frames < 1 || c.enc_tf_window > 512)
            return bad("codec: encoder_dim must be a multiple of 32, 1..8 encoder rates, enc_tf_window <= 512");
        if ((c.encoder_dim << c.n_enc_rates) != c.latent_dim) return bad("codec: latent_dim must be encoder_dim * 2^n_enc_rates");
        for (int i = 0; i < c.n_enc_rates; ++i)
            if (c.enc_tf_layers[i] > 0 && (c.encoder_dim << (i + 1)) % 64) return bad("codec: encoder transformer width must be a multiple of 64");
        if (c.codebook_dim > 16) return bad("codec: codebook_dim <= 16");
        if (c.max_enc_frames > c.max_frames) return bad("codec: max_enc_frames must not exceed max_frames (shared rope table)");
    }
    if (c.max_frames < 1 || c.max_batch < 1) return bad("codec: max_frames / max_batch");
    CodecState* s = new CodecState();
    ctx->codec = s;
    FT_HIP(ctx, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->up_total = 1 << c.n_upsample;
    s->frame_len = s->up_total;
    for (int i = 0; i < c.n_rates; ++i) s->frame_len *= c.rates[i];
    s->has_enc = c.encoder_dim > 0;
    if (s->has_enc) {
        s->hop = 1;
        for (int i = 0; i < c.n_enc_rates; ++i) s->hop *= c.enc_rates[i];
        s->enc_frame_len = s->hop * 4;   // DAC.frame_length (vocoder.py:872)
        s->max_samples = enc_max_samples(c);
    }
    return FT_OK;
}

static void stream_orphan(ft_codec_stream* sc);
static void mix_stream_orphan(ft_mix_stream* ms);
static void room_stream_orphan(ft_room_stream* rs);
static void flac_stream_orphan(ft_flac_stream* fs);
void codec_destroy(ft_ctx* ctx) {
    CodecState* s = ctx->codec;
    if (!s) return;
    if (s->stream) { hipStreamSynchronize(s->stream); hipStreamDestroy(s->stream); }
    // streams the caller has not ended yet: their device state goes with the context, the host handle stays valid for
    // ft_codec_stream_end (which then only deletes it) and is refused by ft_codec_stream_decode
    for (ft_codec_stream* sc : s->streams) stream_orphan(sc);
    s->streams.clear();
    for (ft_mix_stream* ms : s->mix_streams) mix_stream_orphan(ms);
    s->mix_streams.clear();
    for (ft_room_stream* rs : s->room_streams) room_stream_orphan(rs);
    s->room_streams.clear();
    for (ft_flac_stream* fs : s->flac_streams) flac_stream_orphan(fs);
    s->flac_streams.clear();
    for (void* p : s->owned) hipFree(p);
    delete s;
    ctx->codec = nullptr;
}

template <typename T>
static ft_status cmalloc(ft_ctx* ctx, T** p, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, n * sizeof(T) + 64);
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_NOMEM, std::string("codec hipMalloc: ") + hipGetErrorString(e));
    ctx->codec->owned.push_back(q);
    *p = (T*)q;
    return FT_OK;
}
// A table built on the host, to the device on the codec's own stream and waited for: a copy on the legacy stream is refused
// while another thread of the process - a stream's generation - captures a graph on a blocking stream.
static ft_status cupload(ft_ctx* ctx, void* dst, const void* src, size_t bytes) {
    hipStream_t st = ctx->codec->stream;
    FT_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    return FT_OK;
}
static float* W32(ft_ctx* ctx, const std::string& n) { return (float*)ctx->expected[n].p; }
static int gridfor(long n) { long b = (n + 255) / 256; return (int)(b < 4096 ? b : 4096); }

// rows before the current one a convolution reads (a causal convolution's carried rows in a streamed decode)
static int halo_of(const ConvW& w) {
    int h = 0;
    for (int i = 0; i < w.ntap; ++i) h = std::max(h, -w.offs[i]);
    return h;
}
// What the pipelined kernels of gemm() need of a weight: 32-wide K steps, an A stripe of BM + 56 rows.  codec_create's
// channel checks and the convolutions of the model (largest halo 54: k = 7, dilation 9) keep every packed weight to it,
// so gemm()'s fall-back for other weights is never taken ("One decode chain", on why it is still there).
constexpr int GEMM_MAX_HALO = 56;
static ft_status pack_check(ft_ctx* ctx, const ConvW& cw) {
    if (cw.K % 32 == 0 && halo_of(cw) <= GEMM_MAX_HALO) return FT_OK;
    return ft_fail(ctx, FT_ERR_UNSUPPORTED, "codec: a convolution needs input channels in multiples of 32 and a halo of at most 56 rows");
}

static ft_status pack_linear(ft_ctx* ctx, ConvW& cw, const std::string& wname, const std::string& bname, int N, int K) {
    CodecState* s = ctx->codec;
    FT_TRY(cmalloc(ctx, &cw.w, (size_t)N * K));
    pack_rows_kernel<<<gridfor((long)N * K), 256, 0, s->stream>>>(W32(ctx, wname), cw.w, (long)N * K);
    cw.bias = bname.empty() ? nullptr : W32(ctx, bname);
    cw.ntap = 1; cw.N = N; cw.K = K; cw.n_mod = N; cw.offs[0] = 0;
    return pack_check(ctx, cw);
}
static ft_status pack_conv(ft_ctx* ctx, ConvW& cw, const std::string& pfx, int Cout, int Cin, int k, int dil) {
    CodecState* s = ctx->codec;
    FT_TRY(cmalloc(ctx, &cw.w, (size_t)Cout * Cin * k));
    pack_conv_kernel<<<gridfor((long)Cout * Cin * k), 256, 0, s->stream>>>(W32(ctx, pfx + ".weight"), cw.w, Cout, Cin, k);
    cw.bias = W32(ctx, pfx + ".bias");
    cw.ntap = k; cw.N = Cout; cw.K = Cin; cw.n_mod = Cout;
    for (int kk = 0; kk < k; ++kk) cw.offs[kk] = (kk - (k - 1)) * dil;
    return pack_check(ctx, cw);
}
static ft_status pack_convT(ft_ctx* ctx, ConvW& cw, const std::string& pfx, int Cin, int Cout, int k, int stride) {
    CodecState* s = ctx->codec;
    FT_TRY(cmalloc(ctx, &cw.w, (size_t)Cin * Cout * k));
    pack_convT_kernel<<<gridfor((long)Cin * Cout * k), 256, 0, s->stream>>>(W32(ctx, pfx + ".weight"), cw.w, Cin, Cout, k, stride);
    cw.bias = W32(ctx, pfx + ".bias");
    cw.ntap = k / stride; cw.N = stride * Cout; cw.K = Cin; cw.n_mod = Cout;
    for (int j = 0; j < cw.ntap; ++j) cw.offs[j] = -j;
    return pack_check(ctx, cw);
}

static ft_status pack_strided(ft_ctx* ctx, ConvW& cw, const std::string& pfx, int Cout, int Cin, int k, int stride) {
    CodecState* s = ctx->codec;
    FT_TRY(cmalloc(ctx, &cw.w, (size_t)Cout * Cin * k));
    pack_strided_conv_kernel<<<gridfor((long)Cout * Cin * k), 256, 0, s->stream>>>(W32(ctx, pfx + ".weight"), cw.w, Cout, Cin, k, stride);
    cw.bias = W32(ctx, pfx + ".bias");
    cw.ntap = k / stride; cw.N = Cout; cw.K = stride * Cin; cw.n_mod = Cout;
    for (int a = 0; a < cw.ntap; ++a) cw.offs[a] = a - (cw.ntap - 1);
    return pack_check(ctx, cw);
}
static ft_status pack_tf_layer(ft_ctx* ctx, TfLayer& t, const std::string& p, int D, int H, int ffn) {
    CodecState* s = ctx->codec;
    FT_TRY(pack_linear(ctx, t.qkv, p + ".attention.wqkv.weight", "", 3 * H, D));
    FT_TRY(pack_linear(ctx, t.wo, p + ".attention.wo.weight", "", D, H));
    FT_TRY(pack_linear(ctx, t.w2, p + ".feed_forward.w2.weight", "", D, ffn));
    FT_TRY(cmalloc(ctx, &t.w13.w, (size_t)2 * ffn * D));
    pack_interleave_kernel<<<gridfor((long)ffn * D), 256, 0, s->stream>>>(
        W32(ctx, p + ".feed_forward.w1.weight"), W32(ctx, p + ".feed_forward.w3.weight"), t.w13.w, ffn, D);
    t.w13.ntap = 1; t.w13.N = 2 * ffn; t.w13.K = D; t.w13.n_mod = 2 * ffn; t.w13.bias = nullptr;
    t.n1 = W32(ctx, p + ".attention_norm.weight"); t.n2 = W32(ctx, p + ".ffn_norm.weight");
    t.g1 = W32(ctx, p + ".attention_layer_scale.gamma"); t.g2 = W32(ctx, p + ".ffn_layer_scale.gamma");
    return pack_check(ctx, t.w13);
}

// The ConvNeXt block behind the (transposed) convolution of a quantizer.upsample / downsample stage `p`.
static ft_status pack_convnext(ft_ctx* ctx, UpStage& u, const std::string& p, int D) {
    u.f = 2;
    u.dw_w = W32(ctx, p + ".1.dwconv.conv.weight"); u.dw_b = W32(ctx, p + ".1.dwconv.conv.bias");
    u.ln_w = W32(ctx, p + ".1.norm.weight"); u.ln_b = W32(ctx, p + ".1.norm.bias");
    u.gamma = W32(ctx, p + ".1.gamma");
    FT_TRY(pack_linear(ctx, u.pw1, p + ".1.pwconv1.weight", p + ".1.pwconv1.bias", 4 * D, D));
    return pack_linear(ctx, u.pw2, p + ".1.pwconv2.weight", p + ".1.pwconv2.bias", D, 4 * D);
}

static ft_status codec_finalize_encoder(ft_ctx* ctx) {
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    const int D = c.latent_dim, H = c.tf_n_head * c.tf_head_dim, cd = c.codebook_dim, R = c.n_codebooks + 1;
    s->enc_w0 = W32(ctx, "encoder.block.0.conv.weight");
    s->enc_b0 = W32(ctx, "encoder.block.0.conv.bias");
    s->enc.resize(c.n_enc_rates);
    int d = c.encoder_dim;
    long rate = 1, tf_rows = 0;
    int tf_dim = 0;
    for (int i = 0; i < c.n_enc_rates; ++i) {
        CodecState::EncBlock& b = s->enc[i];
        b.cin = d; b.cout = 2 * d; b.s = c.enc_rates[i];
        d *= 2;
        const std::string p = cname("encoder.block.%d.block", i + 1);
        const int dil[3] = {1, 3, 9};
        for (int u = 0; u < 3; ++u) {
            const std::string q = p + cname(".%d.block", u);
            b.u[u].a0 = W32(ctx, q + ".0.alpha"); b.u[u].a2 = W32(ctx, q + ".2.alpha");
            FT_TRY(pack_conv(ctx, b.u[u].c7, q + ".1.conv", b.cin, b.cin, 7, dil[u]));
            FT_TRY(pack_conv(ctx, b.u[u].c1, q + ".3.conv", b.cin, b.cin, 1, 1));
        }
        b.a3 = W32(ctx, p + ".3.alpha");
        FT_TRY(pack_strided(ctx, b.sc, p + ".4.conv", b.cout, b.cin, 2 * b.s, b.s));
        rate *= b.s;
        b.tf.resize(c.enc_tf_layers[i]);
        for (int l = 0; l < c.enc_tf_layers[i]; ++l)
            FT_TRY(pack_tf_layer(ctx, b.tf[l], p + cname(".5.layers.%d", l), b.cout, b.cout, 3 * b.cout));
        if (c.enc_tf_layers[i]) {
            b.tf_norm = W32(ctx, p + ".5.norm.weight");
            tf_rows = std::max(tf_rows, s->max_samples / rate);
            tf_dim = std::max(tf_dim, b.cout);
        }
    }
    s->enc_a_last = W32(ctx, cname("encoder.block.%d.alpha", c.n_enc_rates + 1));
    FT_TRY(pack_conv(ctx, s->enc_out, cname("encoder.block.%d.conv", c.n_enc_rates + 2), D, d, 3, 1));
    s->down.resize(c.n_upsample);
    for (int j = 0; j < c.n_upsample; ++j) {
        const std::string p = cname("quantizer.downsample.%d", j);
        FT_TRY(pack_strided(ctx, s->down[j].ct, p + ".0.conv", D, D, 2, 2));
        FT_TRY(pack_convnext(ctx, s->down[j], p, D));
    }
    s->pre.resize(c.n_tf_layer);
    for (int l = 0; l < c.n_tf_layer; ++l)
        FT_TRY(pack_tf_layer(ctx, s->pre[l], cname("quantizer.pre_module.layers.%d", l), D, H, c.tf_ffn));
    s->pre_norm = W32(ctx, "quantizer.pre_module.norm.weight");
    s->rope_enc = W32(ctx, "rope.codec_enc");
    // quantiser search operands: in_proj (f32), normalised codebooks and their squared norms
    const size_t ncode = (size_t)c.semantic_codebook_size + (size_t)c.n_codebooks * c.codebook_size;
    FT_TRY(cmalloc(ctx, &s->inw, (size_t)R * cd * D));
    FT_TRY(cmalloc(ctx, &s->inb, (size_t)R * cd));
    FT_TRY(cmalloc(ctx, &s->cbn, ncode * cd));
    FT_TRY(cmalloc(ctx, &s->cn2, ncode));
    for (int q = 0; q < R; ++q) {
        const std::string p = q == 0 ? std::string("quantizer.semantic_quantizer.quantizers.0")
                                     : cname("quantizer.quantizer.quantizers.%d", q - 1);
        FT_HIP(ctx, hipMemcpyAsync(s->inw + (size_t)q * cd * D, W32(ctx, p + ".in_proj.weight"), (size_t)cd * D * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
        FT_HIP(ctx, hipMemcpyAsync(s->inb + (size_t)q * cd, W32(ctx, p + ".in_proj.bias"), (size_t)cd * sizeof(float), hipMemcpyDeviceToDevice, s->stream));
        const int N = q == 0 ? c.semantic_codebook_size : c.codebook_size;
        const size_t off = q == 0 ? 0 : (size_t)c.semantic_codebook_size + (size_t)(q - 1) * c.codebook_size;
        normalize_codebook_kernel<<<(N + 255) / 256, 256, 0, s->stream>>>(W32(ctx, p + ".codebook.weight"), s->cbn + off * cd, s->cn2 + off, N, cd);
    }
    // activations: the widest stage is the first (samples x encoder_dim); transformer scratch for the widest transformer
    const size_t big = (size_t)s->max_samples * c.encoder_dim;
    for (int i = 0; i < 4; ++i) FT_TRY(cmalloc(ctx, &s->ebuf[i], std::max(big, (size_t)(s->max_samples / s->hop) * 4 * D)));
    FT_TRY(cmalloc(ctx, &s->enc_audio, (size_t)s->max_samples));
    const size_t rows = std::max<size_t>((size_t)tf_rows, (size_t)c.max_enc_frames);
    const int wd = std::max(tf_dim, D);
    FT_TRY(cmalloc(ctx, &s->enc_x, rows * wd));
    FT_TRY(cmalloc(ctx, &s->e_xn, rows * wd));
    FT_TRY(cmalloc(ctx, &s->e_qkv, rows * 3 * std::max(tf_dim, H)));
    FT_TRY(cmalloc(ctx, &s->e_y, rows * std::max(tf_dim, H)));
    FT_TRY(cmalloc(ctx, &s->e_g, rows * std::max(3 * tf_dim, c.tf_ffn)));
    FT_TRY(cmalloc(ctx, &s->enc_zq, (size_t)c.max_enc_frames * D));
    FT_TRY(cmalloc(ctx, &s->enc_codes, (size_t)R * c.max_enc_frames));
    return FT_OK;
}

ft_status codec_finalize(ft_ctx* ctx) {
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    const int D = c.latent_dim, H = c.tf_n_head * c.tf_head_dim;
    // RVQ tables: out_proj folded into the codebooks (vocoder.py:809-810 + dac from_codes)
    FT_TRY(cmalloc(ctx, &s->tables, ((size_t)c.semantic_codebook_size + (size_t)c.n_codebooks * c.codebook_size) * D));
    {
        const std::string p = "quantizer.semantic_quantizer.quantizers.0";
        rvq_table_kernel<<<gridfor((long)c.semantic_codebook_size * D), 256, 0, s->stream>>>(
            W32(ctx, p + ".codebook.weight"), W32(ctx, p + ".out_proj.weight"), W32(ctx, p + ".out_proj.bias"),
            s->tables, c.semantic_codebook_size, D, c.codebook_dim);
        for (int i = 0; i < c.n_codebooks; ++i) {
            const std::string q = cname("quantizer.quantizer.quantizers.%d", i);
            rvq_table_kernel<<<gridfor((long)c.codebook_size * D), 256, 0, s->stream>>>(
                W32(ctx, q + ".codebook.weight"), W32(ctx, q + ".out_proj.weight"), W32(ctx, q + ".out_proj.bias"),
                s->tables + ((size_t)c.semantic_codebook_size + (size_t)i * c.codebook_size) * D, c.codebook_size, D,
                c.codebook_dim);
        }
    }
    s->rope = W32(ctx, "rope.codec");
    s->tf.resize(c.n_tf_layer);
    for (int l = 0; l < c.n_tf_layer; ++l)
        FT_TRY(pack_tf_layer(ctx, s->tf[l], cname("quantizer.post_module.layers.%d", l), D, H, c.tf_ffn));
    s->tf_norm = W32(ctx, "quantizer.post_module.norm.weight");
    s->up.resize(c.n_upsample);
    for (int j = 0; j < c.n_upsample; ++j) {
        const std::string p = cname("quantizer.upsample.%d", j);
        FT_TRY(pack_convT(ctx, s->up[j].ct, p + ".0.conv", D, D, 2, 2));
        FT_TRY(pack_convnext(ctx, s->up[j], p, D));
    }
    FT_TRY(pack_conv(ctx, s->conv_in, "decoder.model.0.conv", c.decoder_dim, D, 7, 1));
    s->blocks.resize(c.n_rates);
    size_t per_frame_max = (size_t)s->up_total * c.decoder_dim;  // conv_in output
    size_t tmul = s->up_total;
    for (int i = 0; i < c.n_rates; ++i) {
        DecBlock& b = s->blocks[i];
        b.cin = c.decoder_dim >> i; b.cout = c.decoder_dim >> (i + 1); b.s = c.rates[i];
        const std::string p = cname("decoder.model.%d.block", i + 1);
        b.a0 = W32(ctx, p + ".0.alpha");
        FT_TRY(pack_convT(ctx, b.ct, p + ".1.conv", b.cin, b.cout, 2 * b.s, b.s));
        const int dil[3] = {1, 3, 9};
        for (int u = 0; u < 3; ++u) {
            const std::string q = p + cname(".%d.block", u + 2);
            b.u[u].a0 = W32(ctx, q + ".0.alpha"); b.u[u].a2 = W32(ctx, q + ".2.alpha");
            FT_TRY(pack_conv(ctx, b.u[u].c7, q + ".1.conv", b.cout, b.cout, 7, dil[u]));
            FT_TRY(pack_conv(ctx, b.u[u].c1, q + ".3.conv", b.cout, b.cout, 1, 1));
        }
        tmul *= b.s;
        per_frame_max = std::max(per_frame_max, tmul * b.cout);
    }
    s->c_last = c.decoder_dim >> c.n_rates;
    s->a_last = W32(ctx, cname("decoder.model.%d.alpha", c.n_rates + 1));
    {   // [1][C][7] -> [7][C]
        const float* w = W32(ctx, cname("decoder.model.%d.conv.weight", c.n_rates + 2));
        std::vector<float> h((size_t)s->c_last * 7), o((size_t)s->c_last * 7);
        FT_HIP(ctx, hipMemcpy(h.data(), w, h.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int ci = 0; ci < s->c_last; ++ci) for (int k = 0; k < 7; ++k) o[(size_t)k * s->c_last + ci] = h[(size_t)ci * 7 + k];
        FT_TRY(cmalloc(ctx, &s->w_last, o.size()));
        FT_HIP(ctx, hipMemcpy(s->w_last, o.data(), o.size() * sizeof(float), hipMemcpyHostToDevice));
        FT_HIP(ctx, hipMemcpy(&s->b_last, W32(ctx, cname("decoder.model.%d.conv.bias", c.n_rates + 2)), sizeof(float), hipMemcpyDeviceToHost));
    }
    // activation buffers for one utterance of max_frames
    const size_t T = c.max_frames;
    per_frame_max = std::max(per_frame_max, (size_t)s->up_total * 4 * D);  // ConvNeXt hidden
    s->big_elems = T * per_frame_max;
    // 64 rows of the widest conv input in FRONT of every buffer: a streamed decode puts the previous chunk's last rows there
    // (the largest halo is 54 rows: k = 7, dilation 9)
    s->big_margin = (size_t)64 * std::max(c.decoder_dim, D);
    for (int i = 0; i < 4; ++i) {
        FT_TRY(cmalloc(ctx, &s->big[i], s->big_elems + s->big_margin));
        s->big[i] += s->big_margin;
    }
    FT_TRY(cmalloc(ctx, &s->codes, (size_t)(c.n_codebooks + 1) * T));
    FT_TRY(cmalloc(ctx, &s->x, T * D));
    FT_TRY(cmalloc(ctx, &s->xn, T * D));
    FT_TRY(cmalloc(ctx, &s->qkv, (T + (size_t)c.tf_window) * 3 * H));   // (+ window - 1 rows of carried K/V in a streamed decode)
    FT_TRY(cmalloc(ctx, &s->y, T * H));
    FT_TRY(cmalloc(ctx, &s->g, T * c.tf_ffn));
    FT_TRY(cmalloc(ctx, &s->audio, T * s->frame_len));
    if (s->has_enc) FT_TRY(codec_finalize_encoder(ctx));
    FT_HIP(ctx, hipStreamSynchronize(s->stream));
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ launch
struct GemmIO {
    const bf16_t* X; long ldx; int T_in; int M;
    const float* gamma = nullptr; const float* resid_f32 = nullptr; const bf16_t* resid_bf = nullptr; long ldr = 0;
    float* out_f32 = nullptr; bf16_t* out_bf = nullptr; bf16_t* out_act = nullptr; const float* alpha = nullptr;
    long ldo = 0; int act = ACT_NONE;
    long msel = 0;     // rows the kernel VARIANT is chosen for (0 = M): a streamed decode picks, for every chunk length, the variant
                       // a whole utterance of nominal length takes, so that its results do not depend on the chunking
    int t_min = 0;     // TapGemmP::t_min
    // batched streamed decode: nz chunks on blockIdx.z (TapGemmP::seg); M / T_in are then the longest chunk's rows
    const int4* seg = nullptr;
    int nz = 1, seg_m = 1, seg_xg = 0, seg_og = 0;
};

// Returns the id of the instantiation it launched (GEMM_VARIANTS; the launch trace of fishtts_hip_test.h reports it).
struct GemmVariant { const char* name; int bm, bn; };
static const GemmVariant GEMM_VARIANTS[] = {
    {"skinny_gemm<4>", 64, 16},
    {"tapgemm64<64,64,64>", 64, 64}, {"tapgemm64<64,64,32>", 64, 64}, {"tapgemm64<64,96,64>", 64, 96},
    {"tapgemm64<64,96,32>", 64, 96}, {"tapgemm64<128,64,64>", 128, 64}, {"tapgemm64<128,64,32>", 128, 64},
    {"tapgemm64<128,192,32,2,4>", 128, 192}, {"tapgemm64<256,96,32,4,2>", 256, 96}, {"tapgemm64<128,128,64,2,4>", 128, 128},
    {"tapgemm64<128,128,32,2,4>", 128, 128}, {"tapgemm64<128,96,64,4,2>", 128, 96}, {"tapgemm64<128,96,32,4,2>", 128, 96},
    {"tapgemm<128,128,2,2>", 128, 128}, {"tapgemm<128,64,4,1>", 128, 64}};
constexpr int N_GEMM_VARIANTS = (int)(sizeof(GEMM_VARIANTS) / sizeof(GEMM_VARIANTS[0]));

static int gemm(hipStream_t st, const ConvW& w, const GemmIO& io) {
    TapGemmP p{};
    p.X = io.X; p.ldx = io.ldx; p.x_bstride = 0; p.T_in = io.T_in; p.W = w.w; p.ntap = w.ntap;
    for (int i = 0; i < w.ntap; ++i) p.offs[i] = w.offs[i];
    p.M = io.M; p.N = w.N; p.K = w.K; p.bias = w.bias; p.n_mod = w.n_mod; p.act = io.act; p.gamma = io.gamma;
    p.resid_f32 = io.resid_f32; p.resid_bf = io.resid_bf; p.ldr = io.ldr; p.out_f32 = io.out_f32; p.out_bf = io.out_bf;
    p.out_act = io.out_act; p.alpha = io.alpha; p.ldo = io.ldo; p.t_min = io.t_min;
    p.seg = io.seg; p.seg_m = io.seg_m; p.seg_xg = io.seg_xg; p.seg_og = io.seg_og;
    const long Msel = io.msel > 0 ? io.msel : io.M;
    // few rows (the 215-frame transformers, the first up-sampling stage): a 64x64 tile grid leaves most CUs idle and every
    // block walks all of K alone (20-75 us per GEMM); the skinny kernel cuts N into 16-row blocks and splits K over the
    // waves of a block (weights streamed once per 64 rows)
    // (measured per GEMM at 215 / 430 / 860 rows: N = 1024 skinny 8-13 us against 21-75 us; N = 3072 equal; N >= 4096
    // the tile kernel wins, 23 against 35 us: its grid is already >= 256 blocks there)
    constexpr long skinny_m = 1024, skinny_n = 2048;
    if (w.ntap == 1 && w.offs[0] == 0 && Msel <= skinny_m && w.N <= skinny_n && io.T_in >= io.M && w.K % 128 == 0 && w.N % 2 == 0 &&
        (io.act == ACT_NONE || io.act == ACT_SWIGLU || io.act == ACT_GELU) && !io.out_act) {
        p.ldw = 0;
        skinny_gemm_launch<4>(p, (io.M + 63) / 64, st, io.nz);
        return 0;
    }
    if (w.K % 32 == 0 && halo_of(w) <= GEMM_MAX_HALO) {  // pipelined kernel: A stripe shared by the taps, B double-buffered
#define FT_TG(BM_, BN_, BK_)                                                                                   \
    tapgemm64_kernel<BM_, BN_, BK_><<<dim3((io.M + BM_ - 1) / BM_, (w.N + BN_ - 1) / BN_, io.nz), 256,          \
                                      std::max((size_t)((BM_ + 56) + 2 * BN_) * (BK_ + 8) * 2,                  \
                                               (size_t)(BM_ / 2) * (BN_ + 4) * 4), st>>>(p)
        // 64-row tiles on 4 waves below 4096 rows: the 4-wave 128 x 128 instantiation spills registers and, at these sizes,
        // leaves CUs idle (215-frame decode 9.9 -> 6.2 ms)
        const bool vec_ok = io.act != ACT_SWIGLU && w.N % 8 == 0 && w.n_mod % 8 == 0 && io.ldo % 8 == 0 && io.ldr % 8 == 0;
        const bool k64 = w.K % 64 == 0;
        // many rows (the decoder's convolutions after the first up-sampling): 128-row tiles on 8 waves - the 64 x 64 tile is
        // bound by the L2 bandwidth its weight-tile re-reads need (gemm_kernels.h)
#define FT_TG8(BM_, BN_, BK_, NWM_, NWN_)                                                                       \
    do {                                                                                                          \
        constexpr size_t lds8_ = std::max((size_t)((BM_ + 56) + 2 * BN_) * (BK_ + 8) * 2,                         \
                                          (size_t)(BM_ / NWM_) * (BN_ + 4) * 4);                                  \
        static DevOnce once8_;                                                                                    \
        once8_.run([] { hipFuncSetAttribute((const void*)tapgemm64_kernel<BM_, BN_, BK_, NWM_, NWN_>,             \
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds8_); });          \
        tapgemm64_kernel<BM_, BN_, BK_, NWM_, NWN_><<<dim3((io.M + BM_ - 1) / BM_, (w.N + BN_ - 1) / BN_, io.nz), \
                                                      64 * NWM_ * NWN_, lds8_, st>>>(p);                          \
    } while (0)
        constexpr long tile8_m = 4096, wide_m = 30000;
        if (vec_ok && Msel >= tile8_m && (w.N % 128 == 0 || w.N % 96 == 0)) {
            // full-width tiles where the whole N fits one block column (A read once): 128 x 192 (N = 192, 384), 256 x 96 (N = 96)
            // (256 x 128 x 32 on 8 waves was measured slower: 4.76 against 4.57 ms per 215-frame decode)
            if (Msel >= wide_m && w.N % 192 == 0) { FT_TG8(128, 192, 32, 2, 4); return 7; }
            if (Msel >= wide_m && w.N == 96) { FT_TG8(256, 96, 32, 4, 2); return 8; }
            if (w.N % 128 == 0) { if (k64) FT_TG8(128, 128, 64, 2, 4); else FT_TG8(128, 128, 32, 2, 4); return k64 ? 9 : 10; }
            if (k64) FT_TG8(128, 96, 64, 4, 2); else FT_TG8(128, 96, 32, 4, 2);
            return k64 ? 11 : 12;
        }
#undef FT_TG8
        if (w.N % 128 == 0 || (w.N % 96 != 0 && w.N > 96)) {
            if (k64) FT_TG(64, 64, 64); else FT_TG(64, 64, 32);
            return k64 ? 1 : 2;
        } else if (w.N % 96 == 0) {
            if (k64) FT_TG(64, 96, 64); else FT_TG(64, 96, 32);
            return k64 ? 3 : 4;
        } else {
            if (k64) FT_TG(128, 64, 64); else FT_TG(128, 64, 32);
            return k64 ? 5 : 6;
        }
#undef FT_TG
    } else if (w.N >= 128) {   // never taken (pack_check); see there for why the two instantiations stay
        const dim3 grid((io.M + 127) / 128, (w.N + 127) / 128, io.nz);
        tapgemm_kernel<128, 128, 2, 2><<<grid, 256, 0, st>>>(p);
        return 13;
    }
    const dim3 grid((io.M + 127) / 128, (w.N + 63) / 64, io.nz);
    tapgemm_kernel<128, 64, 4, 1><<<grid, 256, 0, st>>>(p);
    return 14;
}

// ---- launch trace (test hook).  A traced call appends one record per launch, in launch order; the launches of the armed
// range also copy what they wrote to the host at that point of the stream (the work buffers are reused later).  The copy
// reads only: a traced call computes what an untraced one does.
struct TraceOut { int kind; const void* p; int f32; };
static std::string tname(const char* fmt, ...) {
    char buf[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}
// m > 0 in a batched streamed call: the rows are those of the chunks back to back, chunk z's at row P_z m + z g of the buffer
// (the gap rows are left out).
static void trace_rec(CodecState* s, hipStream_t st, const std::string& name, long rows, long cols, int variant, int halo, int ntap,
                      int K, std::initializer_list<TraceOut> outs, int m = 0, int g = 0) {
    CodecState::Trace& t = *s->trace;
    const int idx = (int)t.recs.size();
    t.recs.emplace_back();
    CodecState::TraceRec& r = t.recs.back();
    r.name = name; r.rows = (int)rows; r.cols = (int)cols; r.variant = variant; r.halo = halo; r.ntap = ntap; r.K = K;
    r.held = idx >= t.first && idx < t.first + t.count;
    for (const TraceOut& o : outs) {
        if (!o.p) continue;
        r.bufs.emplace_back();
        CodecState::TraceBuf& b = r.bufs.back();
        b.kind = o.kind; b.f32 = o.f32; b.elems = rows * cols;
        if (!r.held) continue;
        const size_t esz = o.f32 ? 4 : 2;
        b.data.resize((size_t)b.elems * esz);
        if (m > 0 && t.batched) {
            char* dst = b.data.data();
            for (size_t z = 0; z < t.chunks.size(); ++z) {
                const size_t nb = (size_t)t.chunks[z].L * m * cols * esz;
                const char* src = (const char*)o.p + ((size_t)t.chunks[z].P * m + z * (size_t)g) * cols * esz;
                if (dst + nb > b.data.data() + b.data.size() || hipMemcpyAsync(dst, src, nb, hipMemcpyDeviceToHost, st) != hipSuccess) { t.failed = true; break; }
                dst += nb;
            }
        } else if (hipMemcpyAsync(b.data.data(), o.p, b.data.size(), hipMemcpyDeviceToHost, st) != hipSuccess) t.failed = true;
    }
    if (r.held && hipStreamSynchronize(st) != hipSuccess) t.failed = true;
}
// The record of a carrying launch of a streamed decode, for chunk z: rows x cols bf16 per buffer, buffer i read at row
// stride ld[i] (kinds 3: the carried rows as placed in front of the chunk, 4: the whole carry left for the next chunk).
struct TraceCarry { int kind; const bf16_t* p; long ld; };
static void trace_carry(CodecState* s, hipStream_t st, const std::string& name, int z, int rows, int cols,
                        std::initializer_list<TraceCarry> outs) {
    CodecState::Trace& t = *s->trace;
    const int idx = (int)t.recs.size();
    t.recs.emplace_back();
    CodecState::TraceRec& r = t.recs.back();
    r.name = name; r.rows = rows; r.cols = cols; r.variant = -1; r.halo = rows; r.ntap = z; r.K = 0;
    r.held = idx >= t.first && idx < t.first + t.count;
    for (const TraceCarry& o : outs) {
        r.bufs.emplace_back();
        CodecState::TraceBuf& b = r.bufs.back();
        b.kind = o.kind; b.f32 = 0; b.elems = (long)rows * cols;
        if (!r.held) continue;
        b.data.resize((size_t)b.elems * 2);
        if (hipMemcpy2DAsync(b.data.data(), (size_t)cols * 2, o.p, (size_t)o.ld * 2, (size_t)cols * 2, (size_t)rows,
                             hipMemcpyDeviceToHost, st) != hipSuccess) t.failed = true;
    }
    if (r.held && hipStreamSynchronize(st) != hipSuccess) t.failed = true;
}
// gemm() and its record: rows x columns as written (a SwiGLU launch writes N / 2 columns; a transposed convolution's
// [M][s * Cout] is the [M * s][Cout] output)
static void gemm_t(CodecState* s, hipStream_t st, const ConvW& w, const GemmIO& io, const char* fmt, int a = 0, int b = 0, const char* pfx = "") {
    const int id = gemm(st, w, io);
    if (s->trace) {
        const long cols = io.act == ACT_SWIGLU ? w.N / 2 : w.N;
        if (io.ldo != cols) s->trace->failed = true;
        trace_rec(s, st, tname(fmt, pfx, a, b), io.seg ? s->trace->frames * io.seg_m : io.M, cols, id, halo_of(w), w.ntap, w.K,
                  {{0, io.out_bf, 0}, {1, io.out_act, 0}, {2, io.out_f32, 1}}, io.seg ? io.seg_m : 0, io.seg_og);
    }
}
struct TraceScope {   // a traced call: armed -> active for this call only
    CodecState* s;
    explicit TraceScope(CodecState* s_, bool eligible) : s(s_) {
        if (!s->tstore.armed) return;
        s->tstore.armed = false;
        if (!eligible) return;
        s->tstore.recs.clear();
        s->tstore.chunks.clear();
        s->tstore.batched = false;
        s->tstore.frames = 0;
        s->tstore.failed = false;
        s->trace = &s->tstore;
    }
    ~TraceScope() { s->trace = nullptr; }
};

// The state checks every codec entry point opens with: a codec in the context and, unless the call works on state that
// only a finalized context hands out (`finalized` false), its weights finalized.
static ft_status codec_ready(ft_ctx* ctx, bool finalized = true) {
    if (!ctx->has_codec || !ctx->codec) return ft_fail(ctx, FT_ERR_STATE, "Vocoder not loaded");
    if (finalized && !ctx->finalized) return ft_fail(ctx, FT_ERR_STATE, "weights not finalized (ft_finalize_weights)");
    return FT_OK;
}

// ---- streamed decode state (ft_codec_stream_*): what the causal codec needs from earlier chunks, two copies of each
// (a chunk reads one and leaves the other).  The codec is strictly causal: the window-128 attention reads the K / V of
// the 127 frames before a chunk (vocoder.py:325-332), every causal convolution the last `halo` rows of its input
// (vocoder.py:411-420, 449-455); with those carried, a chunk's samples are the whole decode's samples, bit for bit.
constexpr int STREAM_NOMINAL_FRAMES = 215;      // kernel variants are those of a 10 s utterance whatever the chunk length
struct ft_codec_stream {
    ft_ctx* owner = nullptr;   // the context whose codec the state belongs to; null once that context is gone (buffers freed)
    int t0 = 0;           // frames decoded so far (rope position of the next chunk's first frame)
    int par = 0;          // which copy is current
    std::vector<bf16_t*> kv[2];                    // per transformer layer: [window - 1][2 * H * hd], newest rows last
    struct Tail { bf16_t* buf[2]; int H, C; };
    std::vector<Tail> tails;                       // in the order decode_chain consumes them
    // the output stages (ft_codec_stream_begin_at / _fx / _fxp; none: the codec's own rate, pace and pitch), each with its
    // carry pair - a call reads one copy and writes the other - and its counters on the host (fx_chain.h)
    StageChain fx;
    bool finished = false;                         // its tail went out (final): no further chunk
    std::vector<void*> owned;
};

static void stream_orphan(ft_codec_stream* sc) {
    for (void* v : sc->owned) hipFree(v);
    sc->owned.clear();
    sc->owner = nullptr;
}

// ---- resampler (RsSeg, resample_kernel; the filter design and rs_ready in fx_chain.h)
constexpr int RS_MAX_SEGS = 64;

// The device table of `rate` (uploaded on its first use); the caller holds s->mu.
static ft_status rs_table(ft_ctx* ctx, int rate, const CodecState::RsTab** out) {
    CodecState* s = ctx->codec;
    auto it = s->rs_tabs.find(rate);
    if (it == s->rs_tabs.end()) {
        CodecState::RsTab t;
        std::vector<float> w;
        if (const char* e = chain::rs_design(rate, &t.L, &t.M, &t.K, &w)) return ft_fail(ctx, FT_ERR_ARG, e);
        if (t.K > 0) {
            FT_TRY(cmalloc(ctx, &t.w, w.size()));
            FT_TRY(cupload(ctx, t.w, w.data(), w.size() * sizeof(float)));
        }
        it = s->rs_tabs.emplace(rate, t).first;
    }
    *out = &it->second;
    return FT_OK;
}

// The output buffer and segment table, allocated once: max_frames of input at the highest rate, plus what streams hold
// back (K/2 L/M + 1 < RS_LDS outputs each).
// `wide`: for time-scaled input (ts_cap samples: twice the codec's, speed 0.5).  A context that resampled before its first
// time-scaled call holds a narrow buffer already: that one is replaced and stays allocated, unused, until the context
// is destroyed (max_frames frame_len 48 / 44.1 floats; the price of allocating nothing wide for callers who never set a speed).
static ft_status rs_alloc(ft_ctx* ctx, bool wide = false) {
    CodecState* s = ctx->codec;
    const size_t in = wide ? s->ts_cap : (size_t)ctx->cc.max_frames * s->frame_len;
    const size_t cap = (in * RS_MAX_RATE + RS_FI - 1) / RS_FI + (size_t)RS_MAX_SEGS * RS_LDS;
    if (s->rs_seg && s->rs_cap >= cap) return FT_OK;
    float* o = nullptr;
    FT_TRY(cmalloc(ctx, &o, cap));
    RsSeg* t = s->rs_seg;
    if (!t) FT_TRY(cmalloc(ctx, &t, (size_t)RS_MAX_SEGS));
    s->rs_out = o;
    s->rs_cap = cap;
    s->rs_seg = t;
    return FT_OK;
}

// ---- time-scale stage (TsSeg, timescale_kernel; fishtts_hip.h states the algorithm, fx_chain.h plans its frames)
// The stage's buffers, allocated once: twice max_frames of audio (speed 0.5) plus what 64 streams can hold back.
static ft_status ts_alloc(ft_ctx* ctx) {
    CodecState* s = ctx->codec;
    if (s->ts_seg) return FT_OK;
    const size_t in = (size_t)ctx->cc.max_frames * s->frame_len;
    const size_t cap = 2 * in + (size_t)RS_MAX_SEGS * (2 * TS_CARRY + 2 * TS_HS);
    std::vector<float> w(TS_N);
    for (int i = 0; i < TS_N; ++i) w[i] = (float)(0.5 * (1.0 - std::cos(2.0 * M_PI * i / TS_N)));
    float *win = nullptr, *o = nullptr;
    int* d = nullptr;
    TsSeg* t = nullptr;
    FT_TRY(cmalloc(ctx, &win, (size_t)TS_N));
    FT_TRY(cupload(ctx, win, w.data(), w.size() * sizeof(float)));
    FT_TRY(cmalloc(ctx, &o, cap));
    FT_TRY(cmalloc(ctx, &d, cap / TS_HS + 2));
    FT_TRY(cmalloc(ctx, &t, (size_t)RS_MAX_SEGS));
    s->ts_win = win;
    s->ts_out = o;
    s->ts_delta = d;
    s->ts_cap = cap;
    s->ts_seg = t;
    return rs_alloc(ctx, true);
}

// ---- pitch stage (PsSeg, pitch_kernel; fishtts_hip.h states it, fx_chain.h designs its table)
// The device table of `cents` (uploaded on its first use); the caller holds s->mu.
static ft_status ps_table(ft_ctx* ctx, int cents, const CodecState::PsTab** out) {
    CodecState* s = ctx->codec;
    auto it = s->ps_tabs.find(cents);
    if (it == s->ps_tabs.end()) {
        CodecState::PsTab t;
        std::vector<float> w;
        if (!chain::ps_design(cents, &t.S, &t.K, &w) || t.K == 0) return ft_fail(ctx, FT_ERR_ARG, "pitch outside [-1200, 1200] cents");
        FT_TRY(cmalloc(ctx, &t.w, w.size()));
        FT_TRY(cupload(ctx, t.w, w.data(), w.size() * sizeof(float)));
        it = s->ps_tabs.emplace(cents, t).first;
    }
    *out = &it->second;
    return FT_OK;
}

// The stage's output buffer (as wide as the time-scale stage's: speed 0.5) and segment table, allocated once, with the
// time-scale stage's buffers (sized for rate 0.5 whatever the call's) and the wide resampler buffer behind them.
static ft_status ps_alloc(ft_ctx* ctx) {
    CodecState* s = ctx->codec;
    FT_TRY(ts_alloc(ctx));
    if (s->ps_seg) return FT_OK;
    float* o = nullptr;
    PsSeg* t = nullptr;
    FT_TRY(cmalloc(ctx, &o, s->ts_cap));
    FT_TRY(cmalloc(ctx, &t, (size_t)RS_MAX_SEGS));
    s->ps_out = o;
    s->ps_seg = t;
    return FT_OK;
}

// ---- level stage (LevelTab and the three kernels in stage_kernels.h; fishtts_hip.h states it, fx_chain.h designs it)
struct LevelJob { int rate = 0, target = 0; ft_level_info* info = nullptr; };   // the level of a one-item call (call_tail)

// A device buffer of at least `need` elements: allocated on first use, replaced by a larger one when a call needs more.
template <typename T>
static ft_status cgrow(ft_ctx* ctx, T** p, size_t* cap, size_t need) {
    CodecState* s = ctx->codec;
    if (*p && *cap >= need) return FT_OK;
    T* q = nullptr;
    FT_TRY(cmalloc(ctx, &q, need + 4));
    if (*p) {
        s->owned.erase(std::find(s->owned.begin(), s->owned.end(), (void*)*p));
        hipFree(*p);
    }
    *p = q;
    *cap = need;
    return FT_OK;
}

static size_t level_hops(long long n, int rate) { return (size_t)((n + chain::lv_hop(rate) - 1) / chain::lv_hop(rate)); }

// The table, and room for `hops` hop sums and peaks.
static ft_status level_alloc(ft_ctx* ctx, size_t hops) {
    CodecState* s = ctx->codec;
    if (!s->lv_tab) FT_TRY(cmalloc(ctx, &s->lv_tab, (size_t)1));
    size_t cap = s->lv_cap;
    FT_TRY(cgrow(ctx, &s->lv_hops, &cap, std::max(hops, (size_t)4)));
    cap = s->lv_cap;
    FT_TRY(cgrow(ctx, &s->lv_peaks, &cap, std::max(hops, (size_t)4)));
    s->lv_cap = cap;
    return FT_OK;
}

// Levels B items in place (x[b], n[b] samples at `rate`, written earlier on the codec's stream), item b toward targets[b]:
// the three launches (two when the call only measures: no target at all, or `scale` false) and the copy of the table back
// to the host.  The caller has called level_alloc for the items' hops, synchronizes, and then reads the results with
// level_fetch.
static ft_status level_enqueue(ft_ctx* ctx, int B, float* const* x, const int64_t* n, int rate, const int* targets, bool scale = true) {
    CodecState* s = ctx->codec;
    hipStream_t st = s->stream;
    s->lv_up.assign(sizeof(LevelTab), 0);
    LevelTab* h = (LevelTab*)s->lv_up.data();
    chain::lv_design(rate, h->c);
    h->ceiling = chain::lv_ceiling();
    h->H = chain::lv_hop(rate);
    h->B = B;
    long long hop0 = 0, most = 0, widest = 0;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        LevelItem& it = h->it[b];
        it.x = x[b];
        it.n = n[b];
        it.hop0 = hop0;
        it.target = targets[b];
        any = any || targets[b] != 0;
        const long long nh = (long long)level_hops(n[b], rate);
        hop0 += nh;
        most = std::max(most, nh);
        widest = std::max(widest, (long long)n[b]);
    }
    if ((size_t)hop0 > s->lv_cap) return ft_fail(ctx, FT_ERR_STATE, "level: hop buffers too small");
    s->lv_nhops = (size_t)hop0;
    const size_t used = offsetof(LevelTab, it) + (size_t)B * sizeof(LevelItem);
    FT_HIP(ctx, hipMemcpyAsync(s->lv_tab, h, used, hipMemcpyHostToDevice, st));
    const int gf = (int)std::max(1LL, (most + LV_FILTER_THREADS - 1) / LV_FILTER_THREADS);
    level_filter_kernel<<<dim3(gf, 1, B), LV_FILTER_THREADS, 0, st>>>(s->lv_tab, s->lv_hops, s->lv_peaks);
    level_gain_kernel<<<B, LV_GAIN_THREADS, 0, st>>>(s->lv_tab, s->lv_hops, s->lv_peaks);
    if (scale && any) {
        const int gx = (int)std::max(1LL, std::min(1024LL, (widest + LV_SCALE_THREADS - 1) / LV_SCALE_THREADS));
        level_scale_kernel<<<dim3(gx, 1, B), LV_SCALE_THREADS, 0, st>>>(s->lv_tab);
    }
    s->lv_down.resize(sizeof(LevelTab));
    FT_HIP(ctx, hipMemcpyAsync(s->lv_down.data(), s->lv_tab, used, hipMemcpyDeviceToHost, st));
    return FT_OK;
}

// Every item toward the call's one target.
static ft_status level_enqueue(ft_ctx* ctx, int B, float* const* x, const int64_t* n, int rate, int target, bool scale = true) {
    int targets[64];
    if (B < 0 || B > 64) return ft_fail(ctx, FT_ERR_STATE, "level: more than 64 items");
    std::fill(targets, targets + B, target);
    return level_enqueue(ctx, B, x, n, rate, targets, scale);
}

// The results of the last level_enqueue, once the stream was synchronized: its item b goes to infos[to ? to[b] : b].  The
// item's target lies in the bytes that pad an ft_level_info: those stay zero, as they always were.
static void level_fetch(CodecState* s, int B, ft_level_info* infos, const int* to = nullptr) {
    const LevelTab* h = (const LevelTab*)s->lv_down.data();
    constexpr size_t told = offsetof(ft_level_info, capped) + sizeof(int32_t);
    for (int b = 0; infos && b < B; ++b) {
        ft_level_info* out = &infos[to ? to[b] : b];
        memcpy(out, &h->it[b].L, told);
        memset((char*)out + told, 0, sizeof(ft_level_info) - told);
    }
}

struct Fx {   // the output stages of a call: resampler segments, and the time-scale and pitch segments in front of some of them
    std::vector<RsSeg> rs;
    std::vector<TsSeg> ts;
    std::vector<PsSeg> ps;
    std::vector<RdSeg> rd;     // the ride stage behind the resampler: none, or one per resampler segment (a call with a live stream)
};

// Time-scales fx.ts (their inputs written earlier on the codec's stream) into ts_out, back to back; segment g's output is
// the input of stream g.rsi's next stage: its pitch segment if it has one, else its resampler segment.
static ft_status ts_enqueue(ft_ctx* ctx, Fx& fx) {
    CodecState* s = ctx->codec;
    std::vector<TsSeg>& segs = fx.ts;
    long long off = 0;
    for (TsSeg& g : segs) {
        g.y = s->ts_out + off;
        const float** in = &fx.rs[g.rsi].x;
        for (PsSeg& q : fx.ps)
            if (q.rsi == g.rsi) in = &q.x;
        *in = g.y;
        off += g.n_out;
    }
    FT_HIP(ctx, hipMemcpyAsync(s->ts_seg, segs.data(), segs.size() * sizeof(TsSeg), hipMemcpyHostToDevice, s->stream));
    timescale_kernel<<<dim3((unsigned)segs.size()), TS_THREADS, 0, s->stream>>>(s->ts_seg, s->ts_win);
    return FT_OK;
}

// Pitch-shifts `segs` (their inputs written earlier on the codec's stream) into ps_out, back to back; segment g's output is
// the input of resampler segment g.rsi.
static ft_status ps_enqueue(ft_ctx* ctx, std::vector<PsSeg>& segs, std::vector<RsSeg>& rs) {
    CodecState* s = ctx->codec;
    long long off = 0, mx = 0;
    for (PsSeg& g : segs) {
        g.y = s->ps_out + off;
        rs[g.rsi].x = g.y;
        off += g.n_out;
        mx = std::max(mx, (long long)g.n_out);
    }
    FT_HIP(ctx, hipMemcpyAsync(s->ps_seg, segs.data(), segs.size() * sizeof(PsSeg), hipMemcpyHostToDevice, s->stream));
    const int gx = (int)std::max(1LL, std::min(2048LL, (mx + RS_THREADS - 1) / RS_THREADS));
    pitch_kernel<<<dim3(gx, 1, (unsigned)segs.size()), RS_THREADS, 0, s->stream>>>(s->ps_seg);
    return FT_OK;
}

// Resamples `segs` (their inputs written earlier on the codec's stream) into rs_out, back to back, and queues the copy of
// all their outputs to `host` (`kind`: a joined call names a device buffer there); the caller synchronizes (and keeps `segs`
// alive until then).  `lv`: the call's one item is levelled in rs_out before the copy.
static ft_status rs_enqueue(ft_ctx* ctx, std::vector<RsSeg>& segs, float* host, hipMemcpyKind kind = hipMemcpyDeviceToHost,
                            const LevelJob* lv = nullptr) {
    CodecState* s = ctx->codec;
    hipStream_t st = s->stream;
    long long off = 0, mx = 0;
    for (RsSeg& g : segs) {
        g.y = s->rs_out + off;
        off += g.n_out;
        mx = std::max(mx, (long long)g.n_out);
    }
    FT_HIP(ctx, hipMemcpyAsync(s->rs_seg, segs.data(), segs.size() * sizeof(RsSeg), hipMemcpyHostToDevice, st));
    const int gx = (int)std::max(1LL, std::min(2048LL, (mx + RS_THREADS - 1) / RS_THREADS));
    resample_kernel<<<dim3(gx, 1, (unsigned)segs.size()), RS_THREADS, 0, st>>>(s->rs_seg);
    if (lv) {
        const int64_t n = off;
        FT_TRY(level_enqueue(ctx, 1, &s->rs_out, &n, lv->rate, lv->target));
    }
    if (off > 0 && host) FT_HIP(ctx, hipMemcpyAsync(host, s->rs_out, (size_t)off * sizeof(float), kind, st));
    return FT_OK;
}

// ---- ride stage (RdSeg and the three kernels in stage_kernels.h; fishtts_hip.h states it, fx_chain.h plans it)
constexpr size_t RD_MAX_HELD = (size_t)(chain::RD_A + 1) * (RS_MAX_RATE / 10);   // a stream holds back less than this

// The segment table and room for `need` emitted samples.
static ft_status rd_alloc(ft_ctx* ctx, size_t need) {
    CodecState* s = ctx->codec;
    if (!s->rd_seg) FT_TRY(cmalloc(ctx, &s->rd_seg, (size_t)RS_MAX_SEGS));
    return cgrow(ctx, &s->rd_out, &s->rd_cap, need);
}

// One stream's ride segment for a call (x: its new samples), from its record and the call's plan; without the stage a copy.
static RdSeg rd_seg_of(const chain::RdStage& r, const chain::RdPlan& q, const float* x) {
    RdSeg g;
    memset(&g, 0, sizeof g);
    g.x = x;
    g.n = (int)q.in;
    g.target = r.target;
    g.H = 1;
    if (r.target == 0) return g;
    g.cin = r.carry[r.par];
    g.cout = r.carry[r.par ^ 1];
    g.e = r.e; g.v = r.v; g.p = r.p; g.g = r.g;
    chain::lv_design(r.rate, g.c);
    g.ceiling = chain::lv_ceiling();
    g.nin = r.nin; g.base = r.base; g.base1 = q.base; g.out0 = r.nout; g.out1 = r.nout + q.out;
    g.H = r.H;
    g.h0 = r.peaks; g.h1 = q.peaks; g.W = q.hops; g.k0 = r.nodes; g.k1 = q.nodes;
    return g;
}

// The ride stage over fx.rd (segment j reads resampler segment j's output) into rd_out, back to back, and the copy of all
// emitted samples to `host`; the caller synchronizes.
static ft_status rd_enqueue(ft_ctx* ctx, Fx& fx, float* host) {
    CodecState* s = ctx->codec;
    hipStream_t st = s->stream;
    long long off = 0, hops = 0, mx = 0;
    bool nodes = false;
    for (size_t j = 0; j < fx.rd.size(); ++j) {
        RdSeg& g = fx.rd[j];
        if (!g.x) g.x = fx.rs[j].y;
        g.y = s->rd_out + off;
        const long long out = g.target != 0 ? g.out1 - g.out0 : g.n;
        off += out;
        hops = std::max(hops, (long long)g.h1 - g.h0);
        nodes = nodes || g.k1 > g.k0;
        mx = std::max({mx, out, g.target != 0 ? g.nin + g.n - g.base1 : 0LL});
    }
    if ((size_t)off > s->rd_cap) return ft_fail(ctx, FT_ERR_STATE, "ride: output buffer too small");
    const unsigned n = (unsigned)fx.rd.size();
    FT_HIP(ctx, hipMemcpyAsync(s->rd_seg, fx.rd.data(), n * sizeof(RdSeg), hipMemcpyHostToDevice, st));
    if (hops > 0) ride_hop_kernel<<<dim3((unsigned)((hops + RD_HOP_THREADS - 1) / RD_HOP_THREADS), 1, n), RD_HOP_THREADS, 0, st>>>(s->rd_seg);
    if (nodes) ride_node_kernel<<<n, RD_NODE_THREADS, 0, st>>>(s->rd_seg);
    if (mx > 0) {
        const int gx = (int)std::min(1024LL, (mx + RD_APPLY_THREADS - 1) / RD_APPLY_THREADS);
        ride_apply_kernel<<<dim3(gx, 1, n), RD_APPLY_THREADS, 0, st>>>(s->rd_seg);
    }
    if (off > 0) FT_HIP(ctx, hipMemcpyAsync(host, s->rd_out, (size_t)off * sizeof(float), hipMemcpyDeviceToHost, st));
    return FT_OK;
}

// ---- the decode chain (DAC.decode), written once.  A Layout says where the rows of a call live; its helpers hand every
// launch site the values that differ between the forms, and the kernels do the rest: they already take one item or the
// chunk of blockIdx.z (SegZ::seg, TapGemmP::seg).
//   one-shot (ft_codec_decode, the encoder's transformers): one item, nothing carried, GEMM variants by the real row count
//   one stream (ft_codec_stream_decode): one chunk; its carries, rope position and carried K/V rows stated by the host
//   many streams (ft_codec_stream_decode_many): n chunks on blockIdx.z; the transformer's per-row stages run on compact
//     rows, everything else leaves gap rows in front of every chunk; what differs per chunk comes from the device table
struct Layout {
    int n = 1;                    // items on blockIdx.z
    const int4* seg = nullptr;    // device table {P, L, t0, nh} per chunk; null: one item
    int T = 0;                    // frames per launch: the item's, or the longest chunk's
    int total = 0;                // frames of all items (the compact rows)
    int own = 0;                  // the item's frames where the host states them; 0: the kernels read them from seg
    int cgap = 0, qgap = 0;       // gap rows in front of every chunk: the convolution buffers, the q k v buffer
    long nominal = 0;             // frames the GEMM variants are chosen for (GemmIO::msel, per frame); 0: the real rows
    const int* codes = nullptr;   // [R][total]
    bf16_t* big[4] = {nullptr, nullptr, nullptr, nullptr};   // convolution work buffers
    bf16_t* qkv = nullptr;        // q k v work buffer, at item 0's first query row
    // carried state.  Carry ci: the convolution tails in the order the chain consumes them, then one K/V per layer
    const std::vector<ft_codec_stream::Tail>* tails = nullptr;   // the list the stream(s) hold; null: nothing carried
    bf16_t* const* hcarry = nullptr;   // one stream: [ncarry][read, write], host pointers handed to the kernels
    bf16_t* const* dcarry = nullptr;   // many: [n][ncarry][read, write] on the device (SegZ::carry)
    bf16_t* const* tcarry = nullptr;   // the launch trace: [n][ncarry][read, write] on the host (one stream: hcarry)
    int ncarry = 0;
    int t0 = 0, nh = 0;           // one stream: rope position, carried K/V rows in front of the chunk (many: from seg)
    int kv_in = 0, kv_out = 0;    // most K/V rows a chunk takes over / leaves behind; 0: no such launch

    static Layout plain(int T, bf16_t* qkv) {
        Layout L;
        L.T = L.total = L.own = T;
        L.qkv = qkv;
        return L;
    }
    int ntail() const { return tails ? (int)tails->size() : 0; }
    dim3 grid(int x) const { return dim3(x, 1, n); }
    // the chunk of blockIdx.z at a stage of m rows per frame and g gap rows (the default SegZ: the one item)
    SegZ Z(int m, int g, int ci = 0) const {
        SegZ z;
        if (seg) { z.seg = seg; z.carry = dcarry; z.ncarry = ncarry; z.ci = ci; z.m = m; z.g = g; }
        return z;
    }
    bf16_t* carry_rd(int ci) const { return hcarry ? hcarry[2 * ci] : nullptr; }
    bf16_t* carry_wr(int ci) const { return hcarry ? hcarry[2 * ci + 1] : nullptr; }
    // a GEMM over every item's rows at m rows per frame; xg / og gap rows in front of every chunk of X / of the output
    GemmIO io(const bf16_t* X, long ldx, int m, int xg, int og) const {
        GemmIO io{X, ldx, T * m, T * m};
        io.msel = nominal * m;
        if (seg) { io.seg = seg; io.nz = n; io.seg_m = m; io.seg_xg = xg; io.seg_og = og; }
        return io;
    }
    // a GEMM over the compact rows of all items (the transformer's linears behind the attention)
    GemmIO io_rows(const bf16_t* X, long ldx) const {
        GemmIO io{X, ldx, total, total};
        io.msel = nominal;
        return io;
    }
};

// One window-limited transformer (vocoder.py:338-354) over the f32 residual stream x [L.total][D]: residual stream f32,
// GEMM operands bf16; the output of the final RMSNorm goes to out_bf and / or out_f32.  A streamed form carries the K / V
// of the window - 1 rows before a chunk (carries L.ntail() + layer).
static void run_transformer(ft_ctx* ctx, const Layout& L, const std::vector<TfLayer>& layers, const float* final_norm,
                            float* x, int D, int H, int hd, int ffn, int window, const float* rope,
                            bf16_t* xn, bf16_t* y, bf16_t* g, bf16_t* out_bf, float* out_f32, const char* pfx) {
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    hipStream_t st = s->stream;
    const int HD = H * hd, W1 = window - 1, T = L.total;
    bf16_t* q0 = L.qkv - (size_t)L.nh * 3 * HD;               // one stream: the carried K/V rows in front of the chunk's
    for (const TfLayer& t : layers) {
        const int l = (int)(&t - layers.data()), ci = L.ntail() + l;
        rmsnorm_rows_kernel<<<T, 256, 0, st>>>(RowNormP{x, t.n1, c.tf_norm_eps, D, xn, nullptr});
        if (s->trace) trace_rec(s, st, tname("%s%d.norm1", pfx, l), T, D, -1, 0, 0, 0, {{0, xn, 0}});
        { GemmIO io = L.io(xn, D, 1, 0, L.qgap); io.out_bf = L.qkv; io.ldo = 3 * HD; gemm_t(s, st, t.qkv, io, "%s%d.qkv", l, 0, pfx); }
        rope_qk_kernel<<<L.grid(gridfor((long)L.T * 2 * H * (hd / 2))), 256, 0, st>>>(L.qkv, rope, L.T, H, hd, L.t0, L.Z(1, L.qgap));
        if (s->trace) trace_rec(s, st, tname("%s%d.rope", pfx, l), T, 3 * HD, -1, 0, 0, 0, {{0, L.qkv, 0}}, 1, L.qgap);
        if (L.kv_in > 0)
            kv_carry_in_kernel<<<L.grid(gridfor((long)L.kv_in * 2 * HD / 8)), 256, 0, st>>>(q0, L.carry_rd(ci), L.nh, W1, HD, L.Z(1, L.qgap, ci));
        if (s->trace && L.kv_in > 0)        // per chunk with carried rows: the k and v thirds of the nh rows in front of it
            for (size_t z = 0; z < s->trace->chunks.size(); ++z) {
                const CodecState::TraceChunk& ch = s->trace->chunks[z];
                const long row0 = s->trace->batched ? (long)ch.P + (long)z * L.qgap : 0;
                if (ch.nh > 0) trace_carry(s, st, tname("%s%d.kvin", pfx, l), (int)z, ch.nh, 2 * HD, {{3, L.qkv + (row0 - ch.nh) * 3 * HD + HD, 3L * HD}});
            }
        if (L.kv_out > 0)
            kv_carry_out_kernel<<<L.grid(gridfor((long)L.kv_out * 2 * HD / 8)), 256, 0, st>>>(
                q0, L.carry_wr(ci), L.nh + L.own, std::min(W1, L.nh + L.own), W1, HD, L.Z(1, L.qgap, ci));
        if (s->trace && L.kv_out > 0)       // per chunk: the whole carry it leaves
            for (size_t z = 0; z < s->trace->chunks.size(); ++z)
                trace_carry(s, st, tname("%s%d.kvout", pfx, l), (int)z, W1, 2 * HD, {{4, L.tcarry[(z * L.ncarry + ci) * 2 + 1], 2L * HD}});
        window_attn_kernel<<<L.grid((L.T * H + 3) / 4), 256, 0, st>>>(
            WinAttnP{q0, y, L.nh + L.own, H, hd, window, 1.0f / sqrtf((float)hd), L.nh, L.Z(1, L.qgap)});
        if (s->trace) trace_rec(s, st, tname("%s%d.attn", pfx, l), T, HD, -1, 0, 0, 0, {{0, y, 0}});
        { GemmIO io = L.io_rows(y, HD); io.gamma = t.g1; io.resid_f32 = x; io.ldr = D; io.out_f32 = x; io.ldo = D; gemm_t(s, st, t.wo, io, "%s%d.wo", l, 0, pfx); }
        rmsnorm_rows_kernel<<<T, 256, 0, st>>>(RowNormP{x, t.n2, c.tf_norm_eps, D, xn, nullptr});
        if (s->trace) trace_rec(s, st, tname("%s%d.norm2", pfx, l), T, D, -1, 0, 0, 0, {{0, xn, 0}});
        { GemmIO io = L.io_rows(xn, D); io.act = ACT_SWIGLU; io.out_bf = g; io.ldo = ffn; gemm_t(s, st, t.w13, io, "%s%d.w13", l, 0, pfx); }
        { GemmIO io = L.io_rows(g, ffn); io.gamma = t.g2; io.resid_f32 = x; io.ldr = D; io.out_f32 = x; io.ldo = D; gemm_t(s, st, t.w2, io, "%s%d.w2", l, 0, pfx); }
    }
    rmsnorm_rows_kernel<<<T, 256, 0, st>>>(RowNormP{x, final_norm, c.tf_norm_eps, D, out_bf, out_f32});
    if (s->trace) trace_rec(s, st, tname("%snorm", pfx), T, D, -1, 0, 0, 0, {{0, out_bf, 0}, {2, out_f32, 1}});
}

// Enqueues the decode of L's rows, RVQ gather to final conv + tanh (the samples land in s->audio, the items back to back).
// false: the carried tails the chain consumes are not the list the stream holds (ft_codec_stream_begin): the call fails.
static bool decode_chain(ft_ctx* ctx, const Layout& L) {
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    hipStream_t st = s->stream;
    const int D = c.latent_dim, G = L.cgap;
    int ti = 0;                                               // next carried tail of *L.tails
    bool in_step = true;
    // the carried rows of x's earlier chunks in front of x (rows [-H, 0)), and the carry for the next chunk; the stream's
    // entry must be this stage's: a stage added here and not there would otherwise read another stage's rows
    // (fmt, a, b: the name of the stage that reads the rows, for the launch trace)
    auto roll = [&](bf16_t* x, int m, int Hh, int C, const char* fmt, int a = 0, int b = 0) {
        if (!L.tails || Hh == 0) return 0;
        if (ti >= L.ntail() || (*L.tails)[ti].H != Hh || (*L.tails)[ti].C != C) { in_step = false; return 0; }
        tail_roll_kernel<<<L.grid(gridfor((long)Hh * C / 8)), 256, 0, st>>>(x, L.carry_rd(ti), L.carry_wr(ti), L.own * m, Hh, C, L.Z(m, G, ti));
        if (s->trace)                       // per chunk: the rows in front of it after the copy, the whole carry it leaves
            for (size_t z = 0; z < s->trace->chunks.size(); ++z) {
                const long row0 = s->trace->batched ? (long)s->trace->chunks[z].P * m + (long)z * G : 0;
                trace_carry(s, st, tname(fmt, a, b), (int)z, Hh, C,
                            {{3, x + (row0 - Hh) * C, (long)C}, {4, L.tcarry[(z * L.ncarry + ti) * 2 + 1], (long)C}});
            }
        ++ti;
        return -Hh;
    };
    RvqP rq{L.codes, s->tables, c.n_codebooks, c.semantic_codebook_size, c.codebook_size, D, L.total, s->x};
    rvq_gather_kernel<<<dim3(L.total, 1), 256, 0, st>>>(rq);
    if (s->trace) trace_rec(s, st, "rvq", L.total, D, -1, 0, 0, 0, {{2, s->x, 1}});
    bf16_t *z = L.big[0], *u = L.big[1], *n = L.big[2], *h = L.big[3];
    run_transformer(ctx, L, s->tf, s->tf_norm, s->x, D, c.tf_n_head, c.tf_head_dim, c.tf_ffn, c.tf_window, s->rope,
                    s->xn, s->y, s->g, z, nullptr, "post.");
    int m = 1, xg = 0;                                        // rows per frame; gap rows of the input (compact after the transformer)
    for (const UpStage& us : s->up) {  // vocoder.py:737-748: convT k=s=2, then ConvNeXt
        const int uj = (int)(&us - s->up.data());
        { GemmIO io = L.io(z, D, m, xg, G / us.f); io.out_bf = u; io.ldo = us.ct.N; gemm_t(s, st, us.ct, io, "%sup.%d.ct", uj); }
        m *= us.f;
        xg = G;
        const int tm = roll(u, m, 6, D, "up.%d.dwln.roll", uj);   // depthwise causal k = 7
        dwconv_ln_kernel<<<L.grid(L.T * m), 256, D * sizeof(float), st>>>(DwLnP{u, us.dw_w, us.dw_b, us.ln_w, us.ln_b, L.T * m, D, n, tm, L.Z(m, G)});
        if (s->trace) trace_rec(s, st, tname("up.%d.dwln", uj), (long)L.total * m, D, -1, 6, 7, 0, {{0, n, 0}}, m, G);
        { GemmIO io = L.io(n, D, m, G, G); io.act = ACT_GELU; io.out_bf = h; io.ldo = 4 * D; gemm_t(s, st, us.pw1, io, "%sup.%d.pw1", uj); }
        { GemmIO io = L.io(h, 4 * D, m, G, G); io.gamma = us.gamma; io.resid_bf = u; io.ldr = D; io.out_bf = z; io.ldo = D; gemm_t(s, st, us.pw2, io, "%sup.%d.pw2", uj); }
    }
    // decoder (vocoder.py:605-640).  Buffers: a = snake'd input of the next conv, r = raw residual
    bf16_t *a = u, *r = n, *hs = h, *a2 = z;
    { GemmIO io = L.io(z, D, m, xg, G); io.out_act = a; io.alpha = s->blocks[0].a0; io.ldo = c.decoder_dim;
      io.t_min = roll(z, m, halo_of(s->conv_in), D, "dec.in.roll"); gemm_t(s, st, s->conv_in, io, "%sdec.in"); }
    // note: conv_in reads z and writes a (= big[1]); z (= big[0]) is free afterwards
    for (size_t bi = 0; bi < s->blocks.size(); ++bi) {
        const DecBlock& b = s->blocks[bi];
        // transposed conv: raw -> r, snake'd by unit 0 -> a2
        { GemmIO io = L.io(a, b.cin, m, G, G / b.s); io.out_bf = r; io.out_act = a2; io.alpha = b.u[0].a0; io.ldo = b.ct.N;
          io.t_min = roll(a, m, halo_of(b.ct), b.cin, "dec.%d.ct.roll", (int)bi); gemm_t(s, st, b.ct, io, "%sdec.%d.ct", (int)bi); }
        m *= b.s;
        for (int ui = 0; ui < 3; ++ui) {
            const ResUnitW& ru = b.u[ui];
            { GemmIO io = L.io(a2, b.cout, m, G, G); io.out_act = hs; io.alpha = ru.a2; io.ldo = b.cout;
              io.t_min = roll(a2, m, halo_of(ru.c7), b.cout, "dec.%d.u%d.c7.roll", (int)bi, ui); gemm_t(s, st, ru.c7, io, "%sdec.%d.u%d.c7", (int)bi, ui); }
            const float* next_alpha = ui < 2 ? b.u[ui + 1].a0 : (bi + 1 < s->blocks.size() ? s->blocks[bi + 1].a0 : s->a_last);
            bf16_t* act_dst = ui < 2 ? a2 : a;  // the last unit feeds the next block's transposed conv / the output conv
            { GemmIO io = L.io(hs, b.cout, m, G, G); io.resid_bf = r; io.ldr = b.cout; io.out_bf = ui < 2 ? r : nullptr;
              io.out_act = act_dst; io.alpha = next_alpha; io.ldo = b.cout; gemm_t(s, st, ru.c1, io, "%sdec.%d.u%d.c1", (int)bi, ui); }
        }
    }
    // m = frame_len here: item z's samples land at P_z * frame_len, back to back as the caller wants them
    FinalConvP fp{a, s->w_last, s->b_last, L.T * m, s->c_last, s->audio, roll(a, m, 6, s->c_last, "final.roll"), L.Z(m, G)};
    final_conv_tanh_kernel<<<L.grid(std::max(16, 2048 / L.n)), 256, 0, st>>>(fp);
    if (s->trace) trace_rec(s, st, "final", (long)L.total * m, 1, -1, 6, 7, s->c_last, {{2, s->audio, 1}});
    return in_step && ti == L.ntail();
}

// The end of a call that leaves samples: the time-scale stage and the resampler over `fx` (inputs written earlier on the stream) or the
// plain copy of `plain` floats of s->audio, the call's one synchronize and the launch check; then every stream named moves
// on by its chunk.  `kind`: where `host` lies (ft_codec_decode_join leaves its items on the device).  `lv`: the level stage
// over the call's one item, behind the last stage and in front of the copy; its result is in lv->info afterwards.
static ft_status call_tail(ft_ctx* ctx, Fx* fx, float* host, size_t plain, const char* what, int n = 0,
                           ft_codec_stream* const* scs = nullptr, const int32_t* lens = nullptr,
                           hipMemcpyKind kind = hipMemcpyDeviceToHost, const LevelJob* lv = nullptr) {
    CodecState* s = ctx->codec;
    if (fx && !fx->ts.empty()) FT_TRY(ts_enqueue(ctx, *fx));
    if (fx && !fx->ps.empty()) FT_TRY(ps_enqueue(ctx, fx->ps, fx->rs));
    if (fx) {
        FT_TRY(rs_enqueue(ctx, fx->rs, fx->rd.empty() ? host : nullptr, kind, lv));
        if (!fx->rd.empty()) FT_TRY(rd_enqueue(ctx, *fx, host));    // the ride stage hands out the call's samples
    } else {
        if (lv) {
            const int64_t np = (int64_t)plain;
            FT_TRY(level_enqueue(ctx, 1, &s->audio, &np, lv->rate, lv->target));
        }
        FT_HIP(ctx, hipMemcpyAsync(host, s->audio, plain * sizeof(float), kind, s->stream));
    }
    FT_HIP(ctx, hipStreamSynchronize(s->stream));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string(what) + hipGetErrorString(e));
    if (lv) level_fetch(s, 1, lv->info);
    for (int j = 0; j < n; ++j) {
        scs[j]->t0 += lens[j];
        scs[j]->par ^= 1;
    }
    return FT_OK;
}

// The chain over L and the end of the call; `who` names the caller in the message of a carry list out of step.
static ft_status decode_run(ft_ctx* ctx, const Layout& L, Fx* rs, float* audio_host, int n,
                            ft_codec_stream* const* scs, const int32_t* lens, const char* who,
                            hipMemcpyKind kind = hipMemcpyDeviceToHost, const LevelJob* lv = nullptr) {
    const bool in_step = decode_chain(ctx, L);
    FT_TRY(call_tail(ctx, rs, audio_host, (size_t)L.total * ctx->codec->frame_len, "codec launch: ", in_step ? n : 0, scs, lens, kind, lv));
    if (!in_step) return ft_fail(ctx, FT_ERR_STATE, std::string(who) + ": carry bookkeeping out of step");
    return FT_OK;
}

// The carries of one stream as the chain numbers them: [read, write] per convolution tail, then per transformer layer.
static void stream_carries(const ft_codec_stream* sc, bf16_t** out) {
    for (const ft_codec_stream::Tail& t : sc->tails) { *out++ = t.buf[sc->par]; *out++ = t.buf[sc->par ^ 1]; }
    for (size_t l = 0; l < sc->kv[0].size(); ++l) { *out++ = sc->kv[sc->par][l]; *out++ = sc->kv[sc->par ^ 1][l]; }
}

// One item: T of the Tfull frames per codebook row of codes_host, decoded from zero state, or (sc) as the next chunk of a
// stream.  `rs`: resample the waveform (segment 0 reads s->audio) and copy the resampled samples instead.  `kind`: the copy
// that delivers the samples (device to device when audio_host is the join stage's input buffer).
static ft_status decode_one(ft_ctx* ctx, const int32_t* codes_host, int Tfull, int T, float* audio_host, ft_codec_stream* sc = nullptr,
                            Fx* rs = nullptr, hipMemcpyKind kind = hipMemcpyDeviceToHost, const LevelJob* lv = nullptr) {
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    const int HD = c.tf_n_head * c.tf_head_dim, R = c.n_codebooks + 1, W1 = c.tf_window - 1;
    Layout L = Layout::plain(T, s->qkv);
    L.codes = s->codes;
    std::copy(s->big, s->big + 4, L.big);
    std::vector<bf16_t*> car;
    if (sc) {
        L.nominal = STREAM_NOMINAL_FRAMES;
        L.tails = &sc->tails;
        L.ncarry = L.ntail() + c.n_tf_layer;
        car.resize((size_t)L.ncarry * 2);
        stream_carries(sc, car.data());
        L.hcarry = L.tcarry = car.data();
        L.t0 = sc->t0;
        L.nh = L.kv_in = std::min(sc->t0, W1);
        L.kv_out = std::min(W1, L.nh + T);
        L.qkv += (size_t)L.nh * 3 * HD;                       // the carried K/V rows go in front
        if (s->trace) { s->trace->chunks.push_back({0, T, L.t0, L.nh}); s->trace->frames = T; }
    }
    // codes of this item, compacted to [R][T]
    std::vector<int> hc((size_t)R * T);
    for (int r = 0; r < R; ++r) memcpy(&hc[(size_t)r * T], codes_host + (size_t)r * Tfull, T * sizeof(int));
    FT_HIP(ctx, hipMemcpyAsync(s->codes, hc.data(), hc.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
    return decode_run(ctx, L, rs, audio_host, sc ? 1 : 0, &sc, &T, "codec stream", kind, lv);
}

// Streamed decode (second half): successive chunks of one utterance's codes, each decoded with
// the context its predecessors left.  The reference decodes every chunk from zero state (synthesizer.py:513-528,
// 591-595: audible restarts at chunk borders); carrying the state is exact because the codec is causal.
extern "C" ft_status ft_codec_stream_begin(ft_ctx* ctx, ft_codec_stream** out) {
    if (!ctx || !out) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    FT_HIP(ctx, hipSetDevice(ctx->device));
    ft_codec_stream* sc = new ft_codec_stream();
    auto zalloc = [&](bf16_t** q, size_t n) -> bool {
        void* v = nullptr;
        if (hipMalloc(&v, n * sizeof(bf16_t) + 64) != hipSuccess) return false;
        sc->owned.push_back(v);
        // on the codec's own (non-blocking) stream: a null-stream memset is not ordered before this context's kernels
        if (hipMemsetAsync(v, 0, n * sizeof(bf16_t) + 64, s->stream) != hipSuccess) return false;
        *q = (bf16_t*)v;
        return true;
    };
    bool ok = true;
    const int HD = c.tf_n_head * c.tf_head_dim, W1 = std::max(c.tf_window - 1, 1);
    for (int k = 0; k < 2 && ok; ++k) {
        sc->kv[k].resize(c.n_tf_layer);
        for (int l = 0; l < c.n_tf_layer && ok; ++l) ok = zalloc(&sc->kv[k][l], (size_t)W1 * 2 * HD);
    }
    auto tail = [&](int Hh, int C) {
        if (Hh == 0 || !ok) return;
        ft_codec_stream::Tail t{{nullptr, nullptr}, Hh, C};
        ok = zalloc(&t.buf[0], (size_t)Hh * C) && zalloc(&t.buf[1], (size_t)Hh * C);
        sc->tails.push_back(t);
    };
    // the order decode_chain consumes them in (its roll() checks every entry against the stage that asks for it)
    for (size_t j = 0; j < s->up.size(); ++j) tail(6, c.latent_dim);
    tail(halo_of(s->conv_in), c.latent_dim);
    for (const DecBlock& b : s->blocks) {
        tail(halo_of(b.ct), b.cin);
        for (int ui = 0; ui < 3; ++ui) tail(halo_of(b.u[ui].c7), b.cout);
    }
    tail(6, s->c_last);
    for (const auto& t : sc->tails) ok = ok && (size_t)t.H * t.C <= s->big_margin && t.C % 8 == 0;
    ok = ok && hipStreamSynchronize(s->stream) == hipSuccess;
    if (!ok) {
        for (void* v : sc->owned) hipFree(v);
        delete sc;
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, "ft_codec_stream_begin: could not set up the carried state");
    }
    sc->owner = ctx;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        s->streams.push_back(sc);
    }
    *out = sc;
    return FT_OK;
}

extern "C" ft_status ft_codec_stream_decode(ft_ctx* ctx, ft_codec_stream* sc, const int32_t* codes, int32_t T, float* audio) {
    if (!ctx || !sc) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx, false));
    if (!codes || !audio || T < 1) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_stream_decode: bad argument");
    if (sc->owner != ctx) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_stream_decode: the stream belongs to another (or a destroyed) context");
    if (sc->fx.rs.tab) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_stream_decode: a stream opened at another sample rate (ft_codec_stream_decode_many_at)");
    if (sc->fx.ts.on) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_stream_decode: a stream opened at another speed (ft_codec_stream_decode_many_at)");
    if (sc->fx.ps.tab) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_stream_decode: a stream opened at another pitch (ft_codec_stream_decode_many_at)");
    if (sc->fx.rd.target != 0) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_stream_decode: a stream opened with a live loudness (ft_codec_stream_decode_many_at)");
    const ft_codec_config& c = ctx->cc;
    if (T > c.max_frames) return ft_fail(ctx, FT_ERR_TOO_LONG, "ft_codec_stream_decode: chunk longer than max_frames");
    if (sc->t0 + T > c.max_frames) return ft_fail(ctx, FT_ERR_TOO_LONG, "ft_codec_stream_decode: stream longer than max_frames (rope table)");
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    TraceScope traced(s, true);
    return decode_one(ctx, codes, T, T, audio, sc);
}

// `ctx` may be null or stale: the stream knows its context, and a stream whose context was destroyed first has no device
// state left (codec_destroy freed it) - only the host handle is deleted then.
extern "C" void ft_codec_stream_end(ft_ctx* ctx, ft_codec_stream* sc) {
    (void)ctx;
    if (!sc) return;
    ft_ctx* own = sc->owner;
    if (own && own->codec) {
        CodecState* s = own->codec;
        std::lock_guard<std::mutex> lock(s->mu);
        hipSetDevice(own->device);
        hipStreamSynchronize(s->stream);
        for (void* v : sc->owned) hipFree(v);
        sc->owned.clear();
        for (size_t i = 0; i < s->streams.size(); ++i)
            if (s->streams[i] == sc) { s->streams.erase(s->streams.begin() + (long)i); break; }
    }
    delete sc;
}

// ---- batched streamed decode (ft_codec_stream_decode_many): one chunk of each of n streams in one pass through the
// codec.  Chunk j holds frames [P_j, P_j + L_j) of the call (P_j = L_0 + .. + L_{j-1}).  The transformer runs on compact
// rows (its norms and linears are per row, the window attention per (query, head)); the q k v work buffer leaves W1 rows
// in front of every chunk for its carried K/V, every convolution buffer MANY_GAP rows for its carried halo rows.  The
// kernels take their chunk from blockIdx.z (TapGemmP::seg, SegZ) and run the arithmetic of ft_codec_stream_decode: the
// variants of the nominal utterance (msel), the same K split and reduction order; only grid extents and row bases change.
// Launches per call do not depend on n.
constexpr int MANY_MAX_STREAMS = 64;
constexpr int MANY_GAP = 64;    // rows in front of every chunk at every convolution stage (largest halo: 54 rows)

static size_t many_seg_bytes() { return (size_t)MANY_MAX_STREAMS * sizeof(int4); }
static size_t many_carry_bytes(int ncarry) { return (size_t)MANY_MAX_STREAMS * ncarry * 2 * sizeof(bf16_t*); }

// The workspace of the batched decode (see fishtts_hip.h for its size), allocated once.
static ft_status many_alloc(ft_ctx* ctx, int ncarry) {
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    if (s->mtab) return FT_OK;
    const int D = c.latent_dim, HD = c.tf_n_head * c.tf_head_dim, W1 = std::max(c.tf_window - 1, 0);
    // widest row of a convolution-stage buffer: the ConvNeXt hidden (4 D), the decoder input (decoder_dim)
    const size_t cmax = std::max({(size_t)4 * D, (size_t)c.decoder_dim, (size_t)D});
    const size_t big = s->big_elems + (size_t)MANY_GAP * (MANY_MAX_STREAMS - 1) * cmax;
    bf16_t* b[4];
    for (int i = 0; i < 4; ++i) FT_TRY(cmalloc(ctx, &b[i], big + s->big_margin));
    bf16_t* q = nullptr;
    FT_TRY(cmalloc(ctx, &q, ((size_t)c.max_frames + (size_t)MANY_MAX_STREAMS * W1) * 3 * HD));
    unsigned char* t = nullptr;
    FT_TRY(cmalloc(ctx, &t, many_seg_bytes() + many_carry_bytes(ncarry) + (size_t)(c.n_codebooks + 1) * c.max_frames * sizeof(int)));
    for (int i = 0; i < 4; ++i) s->mbig[i] = b[i] + s->big_margin;
    s->mqkv = q;
    s->mcarry = ncarry;
    s->mtab = t;    // last: after a failed allocation the workspace stays unset (what was allocated goes with the context)
    return FT_OK;
}

// `rs`: resample the chunks (ft_codec_stream_decode_many_at: the segments' inputs set by the caller) and copy those samples.
static ft_status decode_many(ft_ctx* ctx, int n, ft_codec_stream* const* scs, const int32_t* codes_host, const int32_t* lens,
                             float* audio_host, Fx* rs = nullptr) {
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    const int HD = c.tf_n_head * c.tf_head_dim, R = c.n_codebooks + 1, W1 = c.tf_window - 1;
    const int ncarry = (int)scs[0]->tails.size() + c.n_tf_layer;
    FT_TRY(many_alloc(ctx, ncarry));
    if (s->mcarry != ncarry) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_stream_decode_many: carry count out of step");
    // host side of the device table: chunks {P, L, t0, nh}, carries [n][ncarry][read, write], codes [R][sum L]
    std::vector<int> P(n + 1, 0);
    int Lmax = 0;
    for (int j = 0; j < n; ++j) {
        P[j + 1] = P[j] + lens[j];
        Lmax = std::max(Lmax, (int)lens[j]);
    }
    const int Ts = P[n];
    const size_t seg_b = many_seg_bytes(), car_b = many_carry_bytes(ncarry);
    std::vector<unsigned char> tab(seg_b + car_b + (size_t)R * Ts * sizeof(int));
    int4* seg = reinterpret_cast<int4*>(tab.data());
    bf16_t** car = reinterpret_cast<bf16_t**>(tab.data() + seg_b);
    int* hc = reinterpret_cast<int*>(tab.data() + seg_b + car_b);
    for (int j = 0; j < n; ++j) {
        const ft_codec_stream* sc = scs[j];
        seg[j] = make_int4(P[j], lens[j], sc->t0, std::min(sc->t0, W1));
        stream_carries(sc, car + (size_t)j * ncarry * 2);
        const int32_t* src = codes_host + (size_t)R * P[j];
        for (int r = 0; r < R; ++r) memcpy(hc + (size_t)r * Ts + P[j], src + (size_t)r * lens[j], lens[j] * sizeof(int));
    }
    FT_HIP(ctx, hipMemcpyAsync(s->mtab, tab.data(), tab.size(), hipMemcpyHostToDevice, s->stream));
    Layout L;
    L.n = n; L.T = Lmax; L.total = Ts; L.cgap = MANY_GAP; L.qgap = W1; L.nominal = STREAM_NOMINAL_FRAMES;
    L.seg = reinterpret_cast<const int4*>(s->mtab);
    L.dcarry = reinterpret_cast<bf16_t* const*>(s->mtab + seg_b);
    L.ncarry = ncarry;
    L.tcarry = car;
    if (s->trace) {
        for (int j = 0; j < n; ++j) s->trace->chunks.push_back({seg[j].x, seg[j].y, seg[j].z, seg[j].w});
        s->trace->batched = true;
        s->trace->frames = Ts;
    }
    L.codes = reinterpret_cast<const int*>(s->mtab + seg_b + car_b);
    std::copy(s->mbig, s->mbig + 4, L.big);
    // chunk z's q k v rows start at row P_z + z * W1 of L.qkv (its carried K/V in front)
    L.qkv = s->mqkv + (size_t)W1 * 3 * HD;
    L.tails = &scs[0]->tails;                                 // all streams of a context hold the same list
    L.kv_in = L.kv_out = std::max(W1, 0);
    return decode_run(ctx, L, rs, audio_host, n, scs, lens, "ft_codec_stream_decode_many");
}

// What ft_codec_stream_decode_many and .._many_at refuse, in one order: `fn` names the function in the message; `at`
// (the second) takes streams of any rate that are not finished and, with `final`, a chunk of no frames.
static ft_status many_check(ft_ctx* ctx, const std::string& fn, int n, ft_codec_stream* const* streams, const int32_t* lens,
                            const int32_t* final, bool at) {
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    if (n > MANY_MAX_STREAMS) return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": more than 64 streams in one call");
    if (s->up.empty()) return ft_fail(ctx, FT_ERR_UNSUPPORTED, fn + ": needs an up-sampling stage");
    for (const DecBlock& b : s->blocks)
        if (MANY_GAP % b.s) return ft_fail(ctx, FT_ERR_UNSUPPORTED, fn + ": decoder rates must divide 64");
    long total = 0;
    for (int j = 0; j < n; ++j) {
        const ft_codec_stream* sc = streams[j];
        if (!sc) return ft_fail(ctx, FT_ERR_ARG, fn + ": null stream");
        if (lens[j] < 0 || (lens[j] == 0 && !(at && final && final[j])))
            return ft_fail(ctx, FT_ERR_ARG, fn + ": a chunk of less than one frame" + (at ? " (zero only with final)" : ""));
        if (sc->owner != ctx) return ft_fail(ctx, FT_ERR_STATE, fn + ": a stream belongs to another (or a destroyed) context");
        if (!at && sc->fx.rs.tab) return ft_fail(ctx, FT_ERR_STATE, fn + ": a stream opened at another sample rate (ft_codec_stream_decode_many_at)");
        if (!at && sc->fx.ts.on) return ft_fail(ctx, FT_ERR_STATE, fn + ": a stream opened at another speed (ft_codec_stream_decode_many_at)");
        if (!at && sc->fx.ps.tab) return ft_fail(ctx, FT_ERR_STATE, fn + ": a stream opened at another pitch (ft_codec_stream_decode_many_at)");
        if (!at && sc->fx.rd.target != 0) return ft_fail(ctx, FT_ERR_STATE, fn + ": a stream opened with a live loudness (ft_codec_stream_decode_many_at)");
        if (at && sc->finished) return ft_fail(ctx, FT_ERR_STATE, fn + ": a stream whose final chunk went out");
        for (int i = 0; i < j; ++i)
            if (streams[i] == sc) return ft_fail(ctx, FT_ERR_ARG, fn + ": a stream named twice");
        if (lens[j] > c.max_frames || sc->t0 + lens[j] > c.max_frames)
            return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": stream longer than max_frames (rope table)");
        total += lens[j];
    }
    if (total > c.max_frames) return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": chunks longer than max_frames together");
    return FT_OK;
}

extern "C" ft_status ft_codec_stream_decode_many(ft_ctx* ctx, int32_t n, ft_codec_stream* const* streams, const int32_t* codes,
                                                 const int32_t* lens, float* audio) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (n < 1 || !streams || !codes || !lens || !audio) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_stream_decode_many: bad argument");
    FT_TRY(many_check(ctx, "ft_codec_stream_decode_many", n, streams, lens, nullptr, false));
    std::lock_guard<std::mutex> lock(ctx->codec->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    TraceScope traced(ctx->codec, true);
    return decode_many(ctx, n, streams, codes, lens, audio);
}

// The segments of one waveform's stages for a call: `x` holds the call's codec samples, `j` is the waveform's place in the
// call (its resampler segment, which every waveform has: the copy out), `deltas` the test hooks' d_k.  A stage reads the
// current copy of its carry and writes the other; ts_enqueue and ps_enqueue point the later stages at the earlier ones' output.
// `ride`: the call has a live stream, and every waveform gets a ride segment behind its resampler segment (a copy without the stage).
static void chain_segs(const StageChain& c, const ChainPlan& p, const float* x, int j, int* deltas, Fx& fx, bool ride = false) {
    const chain::TsStage& t = c.ts;
    if (t.on)
        fx.ts.push_back(TsSeg{x, t.carry[t.par], t.carry[t.par ^ 1], t.state[t.par], t.state[t.par ^ 1], nullptr, deltas, t.nin, t.base,
                              p.ts.base, t.nout, t.rate.num, t.rate.den, (int)p.ts.in, (int)p.ts.out, t.k, p.ts.k1, j, 0});
    const chain::PsStage& q = c.ps;
    if (q.tab)
        fx.ps.push_back(PsSeg{x, q.tab->w, q.carry[q.par], q.carry[q.par ^ 1], nullptr, q.nin, q.nout, q.tab->S, (int)p.ps.in,
                              (int)p.ps.out, q.tab->K, j});
    const chain::RsStage& r = c.rs;
    fx.rs.push_back(RsSeg{x, nullptr, r.carry[r.par], r.carry[r.par ^ 1], nullptr, r.nin, r.nout, (int)p.rs.in, (int)p.rs.out, 1, 1, 0, 0});
    if (r.tab) { RsSeg& g = fx.rs.back(); g.w = r.tab->w; g.L = r.tab->L; g.M = r.tab->M; g.K = r.tab->K; }
    if (ride) fx.rd.push_back(rd_seg_of(c.rd, p.rd, nullptr));   // (rd_enqueue points it at the resampler segment's output)
}

// The output stages of one item of n_in codec samples decoded from zero state: a fresh input to each stage, zeros before
// it, zeros after it (the whole tail).  False: no stage at all (the codec's own rate, pace and pitch).
static bool item_stages(CodecState* s, const FxDesc& d, long long n_in, Fx& g) {
    if (!d.any()) return false;
    const StageChain c = d.fresh();
    chain_segs(c, c.plan(n_in, true), s->audio, 0, nullptr, g);
    return true;
}

// The items of ft_codec_decode / ft_codec_decode_fxp, one after the other through the chain `d`: item b's samples go to
// audio + b * stride, zeros behind them.  With a level (d.level), every item is levelled before its copy; infos[b] (infos
// may be null) receives what the stage found, an item without samples the result of an empty one.
static ft_status decode_items(ft_ctx* ctx, const std::string& fn, const int32_t* codes, int B, int T, const int32_t* lens, float* audio,
                              size_t stride, const FxDesc& d, int64_t* out_lens, ft_level_info* infos = nullptr) {
    CodecState* s = ctx->codec;
    const int R = ctx->cc.n_codebooks + 1;
    for (int b = 0; b < B; ++b) {
        const int Tb = lens ? lens[b] : T;
        if (Tb < 0 || Tb > T) return ft_fail(ctx, FT_ERR_ARG, fn + ": bad length");
        const long long n_in = (long long)Tb * s->frame_len;
        const size_t n_out = (size_t)d.out_len(n_in);
        float* out = audio + (size_t)b * stride;
        if (out_lens) out_lens[b] = (int64_t)n_out;
        if (n_out < stride) memset(out + n_out, 0, (stride - n_out) * sizeof(float));
        ft_level_info info = {-INFINITY, 0.f, 1.f, 0, 0, 0};
        if (infos) infos[b] = info;
        if (Tb == 0) continue;
        Fx g;
        const bool staged = item_stages(s, d, n_in, g);
        const LevelJob lv{d.rate, d.level, &info};
        FT_TRY(decode_one(ctx, codes + (size_t)b * R * T, T, Tb, out, nullptr, staged ? &g : nullptr, hipMemcpyDeviceToHost,
                          d.level != 0 ? &lv : nullptr));
        if (infos) infos[b] = info;
    }
    return FT_OK;
}

extern "C" ft_status ft_codec_decode(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                     float* audio) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!codes || !audio || B < 1 || T < 1) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_decode: bad argument");
    if (T > ctx->cc.max_frames) return ft_fail(ctx, FT_ERR_TOO_LONG, "ft_codec_decode: T exceeds max_frames");
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    TraceScope traced(s, B == 1);
    return decode_items(ctx, "ft_codec_decode", codes, B, T, lens, audio, (size_t)T * s->frame_len, FxDesc(), nullptr);
}

// ---- resampled output (fishtts_hip.h: ft_resample_filter .. ft_codec_stream_decode_many_at, ft_test_resample)
extern "C" ft_status ft_resample_filter(int32_t sample_rate, int32_t* L, int32_t* M, int32_t* K, float* table) {
    int l = 1, m = 1, k = 0;
    std::vector<float> w;
    if (chain::rs_design(sample_rate, &l, &m, &k, table ? &w : nullptr)) return FT_ERR_ARG;
    if (L) *L = l;
    if (M) *M = m;
    if (K) *K = k;
    if (table && !w.empty()) memcpy(table, w.data(), w.size() * sizeof(float));
    return FT_OK;
}

extern "C" int64_t ft_resampled_len(int32_t sample_rate, int64_t n_in) {
    int l = 1, m = 1, k = 0;
    if (n_in < 0 || chain::rs_design(sample_rate, &l, &m, &k, nullptr)) return -1;
    return (n_in * l + m - 1) / m;
}

// A call's chain from its three values, judged without a lock and before anything else: the rate, then the speed, then
// the cents, then the pair, then the level, then the ride stage's target.  `fn` names the entry point in the message.
static ft_status fx_refuse(ft_ctx* ctx, const std::string& fn, int rate, int pct, int cents, FxDesc* d, int level = 0, int live = 0) {
    const char* why = nullptr;
    switch (d->make(rate, pct, cents, level, live, &why)) {
    case FxDesc::RATE: return ft_fail(ctx, FT_ERR_ARG, fn + ": " + why + " (" + std::to_string(rate) + ")");
    case FxDesc::SPEED: return ft_fail(ctx, FT_ERR_ARG, fn + ": speed outside [50, 200] percent (" + std::to_string(pct) + ")");
    case FxDesc::CENTS: return ft_fail(ctx, FT_ERR_ARG, fn + ": pitch outside [-1200, 1200] cents (" + std::to_string(cents) + ")");
    case FxDesc::PAIR:
        return ft_fail(ctx, FT_ERR_ARG, fn + ": speed / pitch ratio outside [0.5, 2] (speed " + std::to_string(pct) + " percent, " +
                                            std::to_string(cents) + " cents)");
    case FxDesc::LEVEL:
        return ft_fail(ctx, FT_ERR_ARG, fn + ": loudness outside [-5000, -500] hundredths of a LUFS (" + std::to_string(level) + ")");
    case FxDesc::LIVE:
        return ft_fail(ctx, FT_ERR_ARG, fn + ": live loudness outside [-5000, -500] hundredths of a LUFS (" + std::to_string(live) + ")");
    case FxDesc::OK: break;
    }
    return FT_OK;
}

// The chain's device side; the caller holds s->mu.  The tables of its rate and cents, and the buffers of the first stage it
// has (each stage's allocation brings those of the stages behind it); with a level, the level stage's table and `hops` hop sums.
// `count` chains of one call (at most 64, all at one rate): the union of theirs (item_fx.h) - every distinct cents value's
// table, the buffers of the longest chain, `hops` hop sums for those with a level.
static ft_status fx_prepare(ft_ctx* ctx, FxDesc* d, size_t hops = 0, int count = 1) {
    if (count < 1 || count > JOIN_MAX_ITEMS) return ft_fail(ctx, FT_ERR_STATE, "fx_prepare: 1 to 64 chains");
    const ItemFxUnion u = item_fx_union(d, count, nullptr);
    bool live = false;       // (a stream's; such a call has one chain)
    for (int i = 0; i < count; ++i) live = live || d[i].live != 0;
    if (u.levelled > 0) FT_TRY(level_alloc(ctx, hops));
    FT_TRY(rs_table(ctx, d[0].rate, &d[0].rs));
    const CodecState::PsTab* ps[JOIN_MAX_ITEMS];
    for (int k = 0; k < u.ncents; ++k) FT_TRY(ps_table(ctx, u.cents[k], &ps[k]));
    for (int i = 0; i < count; ++i) {
        d[i].rs = d[0].rs;
        if (d[i].cents != 0) d[i].ps = ps[std::find(u.cents, u.cents + u.ncents, d[i].cents) - u.cents];
    }
    if (u.ps) {
        FT_TRY(ps_alloc(ctx));
    } else if (u.ts) {
        FT_TRY(ts_alloc(ctx));
    } else if (u.rs || live) {
        FT_TRY(rs_alloc(ctx));       // (a live stream's samples pass through the resampler's buffer at any rate)
    }
    // a live stream: everything a call's resampler can give, and what 64 streams can hold back
    // (kept in step with the resampler's buffer once the context has had a live stream: a later chain may widen that one)
    return live || ctx->codec->rd_seg ? rd_alloc(ctx, ctx->codec->rs_cap + (size_t)RS_MAX_SEGS * RD_MAX_HELD) : FT_OK;
}

extern "C" int64_t ft_timescaled_len(int32_t speed_pct, int64_t n_in) {
    return n_in < 0 || !chain::ts_ok(speed_pct) ? -1 : chain::ts_len(speed_pct, n_in);
}

extern "C" ft_status ft_pitch_filter(int32_t cents, int64_t* step, int32_t* K, float* table) {
    long long S = 0;
    int k = 0;
    std::vector<float> w;
    if (!chain::ps_design(cents, &S, &k, table ? &w : nullptr)) return FT_ERR_ARG;
    if (step) *step = S;
    if (K) *K = k;
    if (table && !w.empty()) memcpy(table, w.data(), w.size() * sizeof(float));
    return FT_OK;
}

extern "C" ft_status ft_pitch_ok(int32_t speed_pct, int32_t cents) { return chain::fx_plan(speed_pct, cents, nullptr) ? FT_OK : FT_ERR_ARG; }

static ft_status decode_fx(ft_ctx* ctx, const std::string& fn, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                           int32_t sample_rate, int32_t pct, float* audio, int64_t* out_lens, int32_t cents = 0, int32_t level = 0,
                           ft_level_info* infos = nullptr) {
    if (!ctx) return FT_ERR_ARG;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, fn, sample_rate, pct, cents, &d, level));
    FT_TRY(codec_ready(ctx));
    if (!codes || !audio || !out_lens || B < 1 || T < 1) return ft_fail(ctx, FT_ERR_ARG, fn + ": bad argument");
    if (T > ctx->cc.max_frames) return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": T exceeds max_frames");
    CodecState* s = ctx->codec;
    int64_t stride = 0;   // the longest item's output length (a bad length is refused before the table is built)
    for (int b = 0; b < B; ++b) {
        const int Tb = lens ? lens[b] : T;
        if (Tb < 0 || Tb > T) return ft_fail(ctx, FT_ERR_ARG, fn + ": bad length");
        stride = std::max(stride, (int64_t)d.out_len((long long)Tb * s->frame_len));
    }
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_TRY(fx_prepare(ctx, &d, level_hops(stride, d.rate)));     // (one item at a time: the longest one's hops)
    return decode_items(ctx, fn, codes, B, T, lens, audio, (size_t)stride, d, out_lens, infos);
}

extern "C" ft_status ft_codec_decode_at(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                        int32_t sample_rate, float* audio, int64_t* out_lens) {
    return decode_fx(ctx, "ft_codec_decode_at", codes, B, T, lens, sample_rate, 100, audio, out_lens);
}

extern "C" ft_status ft_codec_decode_fx(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                        int32_t sample_rate, int32_t speed_pct, float* audio, int64_t* out_lens) {
    return decode_fx(ctx, "ft_codec_decode_fx", codes, B, T, lens, sample_rate, speed_pct, audio, out_lens);
}

extern "C" ft_status ft_codec_decode_fxp(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                         int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents, float* audio, int64_t* out_lens) {
    return decode_fx(ctx, "ft_codec_decode_fxp", codes, B, T, lens, sample_rate, speed_pct, audio, out_lens, pitch_cents);
}

extern "C" ft_status ft_codec_decode_level(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                           int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents, int32_t loudness, float* audio,
                                           int64_t* out_lens, ft_level_info* infos) {
    return decode_fx(ctx, "ft_codec_decode_level", codes, B, T, lens, sample_rate, speed_pct, audio, out_lens, pitch_cents, loudness, infos);
}

// ---- level stage alone (fishtts_hip.h: ft_level_filter, ft_codec_loudness; fishtts_hip_test.h: ft_test_level_hops)
extern "C" ft_status ft_level_filter(int32_t sample_rate, double* coeffs, int32_t* hop) {
    int l = 1, m = 1, k = 0;
    if (chain::rs_design(sample_rate, &l, &m, &k, nullptr)) return FT_ERR_ARG;
    if (coeffs) chain::lv_design(sample_rate, coeffs);
    if (hop) *hop = chain::lv_hop(sample_rate);
    return FT_OK;
}

extern "C" ft_status ft_codec_loudness(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, int32_t target,
                                       ft_level_info* info, float* y) {
    const std::string fn = "ft_codec_loudness";
    if (!ctx) return FT_ERR_ARG;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, fn, sample_rate, 100, 0, &d, target));
    FT_TRY(codec_ready(ctx));
    if ((!x && n > 0) || !info || n < 0) return ft_fail(ctx, FT_ERR_ARG, fn + ": bad argument");
    CodecState* s = ctx->codec;
    // the longest item a decode can give: max_frames of audio at speed 0.5 and the highest rate
    const int64_t most = (2 * (int64_t)ctx->cc.max_frames * s->frame_len * RS_MAX_RATE + RS_FI - 1) / RS_FI;
    if (n > most) return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": longer than the longest item a decode gives");
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_TRY(level_alloc(ctx, level_hops(n, sample_rate)));
    FT_TRY(cgrow(ctx, &s->lv_x, &s->lv_xcap, (size_t)std::max(n, (int64_t)4)));
    if (n > 0) FT_HIP(ctx, hipMemcpyAsync(s->lv_x, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    FT_TRY(level_enqueue(ctx, 1, &s->lv_x, &n, sample_rate, target, y != nullptr));
    if (y && n > 0) FT_HIP(ctx, hipMemcpyAsync(y, s->lv_x, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    FT_HIP(ctx, hipStreamSynchronize(s->stream));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("level launch: ") + hipGetErrorString(e));
    level_fetch(s, 1, info);
    return FT_OK;
}

extern "C" ft_status ft_test_level_hops(ft_ctx* ctx, double* hops, int64_t capacity, int64_t* count) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!count || (capacity > 0 && !hops)) return ft_fail(ctx, FT_ERR_ARG, "ft_test_level_hops: bad argument");
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    *count = (int64_t)s->lv_nhops;
    const size_t k = std::min((size_t)std::max(capacity, (int64_t)0), s->lv_nhops);
    if (k > 0) FT_HIP(ctx, hipMemcpy(hops, s->lv_hops, k * sizeof(double), hipMemcpyDeviceToHost));
    return FT_OK;
}

// ---- join stage (fishtts_hip.h: ft_codec_decode_join; JoinTab and the three kernels in stage_kernels.h, the argument
// checks and the layout of the input buffer in join_plan.h)
// Room for `in` input and `out` output samples: allocated on the first call, replaced by larger buffers when a call needs more.
static ft_status join_alloc(ft_ctx* ctx, size_t in, size_t out) {
    CodecState* s = ctx->codec;
    if (!s->join_tab) FT_TRY(cmalloc(ctx, &s->join_tab, (size_t)1));
    auto grow = [&](float** p, size_t* cap, size_t need) -> ft_status {
        if (*p && *cap >= need) return FT_OK;
        float* q = nullptr;
        FT_TRY(cmalloc(ctx, &q, need + 4));
        if (*p) {
            s->owned.erase(std::find(s->owned.begin(), s->owned.end(), (void*)*p));
            hipFree(*p);
        }
        *p = q;
        *cap = need;
        return FT_OK;
    };
    FT_TRY(grow(&s->join_in, &s->join_in_cap, std::max(in, (size_t)4)));
    return grow(&s->join_out, &s->join_out_cap, std::max(out, (size_t)4));
}

// The three launches over items that lie at join_in + off[b] (written earlier on the codec's stream), then the table's
// head - total and the cuts - and `*total` samples to the host.  `fill`: the test hook's form - the output buffer pre-filled with the sentinel and all
// `need` samples of it copied back.  `fetch` false: the call stops after the one read-back of total and the cuts, the pieces
// stay in join_out for a stage behind the join (the intake's encoder).
static ft_status join_run(ft_ctx* ctx, int B, const int64_t* n, const int64_t* off, const ft_join_params* jp, const int64_t* gaps,
                          int started, float* audio, int64_t* total, int64_t* cuts, int64_t need, bool fill, bool fetch = true) {
    CodecState* s = ctx->codec;
    hipStream_t st = s->stream;
    std::vector<char> raw(sizeof(JoinTab));
    JoinTab* h = (JoinTab*)raw.data();
    memset(h, 0, sizeof(JoinTab));
    h->started = started;
    h->B = B;
    long long widest = 0;
    for (int b = 0; b < B; ++b) {
        JoinItem& it = h->it[b];
        it.x = s->join_in + off[b];
        it.n = n[b];
        it.gap = gaps[b];
        it.first = INT_MAX;
        it.last = -1;
        widest = std::max(widest, (long long)(n[b] + gaps[b]));
    }
    const size_t used = offsetof(JoinTab, it) + (size_t)B * sizeof(JoinItem);
    FT_HIP(ctx, hipMemcpyAsync(s->join_tab, h, used, hipMemcpyHostToDevice, st));
    if (fill && need > 0) FT_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)s->join_out, (int)0xFFFFFFFE, (size_t)need, st));
    const int gx = (int)std::max(1LL, std::min(1024LL, (widest / 4 + JOIN_THREADS - 1) / JOIN_THREADS));
    join_edges_kernel<<<dim3(std::min(gx, JOIN_EDGE_BLOCKS), 1, B), JOIN_THREADS, 0, st>>>(s->join_tab, jp->threshold, jp->hop);
    join_layout_kernel<<<1, 64, 0, st>>>(s->join_tab, jp->hop, jp->keep, jp->fade);
    join_assemble_kernel<<<dim3(gx, 1, B), JOIN_THREADS, 0, st>>>(s->join_tab, s->join_out);
    FT_HIP(ctx, hipMemcpyAsync(h, s->join_tab, offsetof(JoinTab, started), hipMemcpyDeviceToHost, st));   // total and the cuts
    FT_HIP(ctx, hipStreamSynchronize(st));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("join launch: ") + hipGetErrorString(e));
    if (h->total < 0 || h->total > need) return ft_fail(ctx, FT_ERR_STATE, "join: layout out of range");
    const int64_t ncopy = fill ? need : (int64_t)h->total;
    if (ncopy > 0 && fetch) {       // its length is known only now: the call's second and last wait
        FT_HIP(ctx, hipMemcpyAsync(audio, s->join_out, (size_t)ncopy * sizeof(float), hipMemcpyDeviceToHost, st));
        FT_HIP(ctx, hipStreamSynchronize(st));
    }
    *total = h->total;
    memcpy(cuts, h->cuts, (size_t)B * 2 * sizeof(int64_t));
    return FT_OK;
}

extern "C" int32_t ft_join_groups(const int32_t* lens, int32_t n, int32_t max_frames, int32_t* ends) {
    return join_groups(lens, n, max_frames, ends);
}

// ft_codec_decode_join, ft_codec_decode_join_level and ft_codec_decode_join_items: the items decoded one after the other into
// join_in, each through its own chain, those with a level levelled there in one go (the item is a grid dimension), then
// joined.  `per_item`: fx has B entries and the refusals name the item (item_fx.h); else fx is the one chain of all items.
static ft_status decode_join(ft_ctx* ctx, const std::string& fn, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                             int32_t sample_rate, const ft_item_fx* fx, bool per_item, const ft_join_params* jp,
                             const int64_t* gaps, int32_t started, float* audio, int64_t capacity, int64_t* total,
                             int64_t* cuts, ft_level_info* infos) {
    if (!ctx) return FT_ERR_ARG;
    FxDesc d[JOIN_MAX_ITEMS];
    if (per_item) {
        FT_TRY(fx_refuse(ctx, fn, sample_rate, 100, 0, &d[0]));       // the rate, which the items share, first
        if (!fx || B < 1 || B > JOIN_MAX_ITEMS) return ft_fail(ctx, FT_ERR_ARG, fn + ": bad argument");
        const ItemFxBad bad = item_fx_make(sample_rate, fx, B, d);
        if (bad.bad != FxDesc::OK) {       // (fx_refuse words the message; it judges the item again, to the same end)
            const ft_item_fx& f = fx[bad.item];
            const ft_status st = fx_refuse(ctx, fn + ": item " + std::to_string(bad.item), sample_rate, f.speed_pct, f.pitch_cents, &d[0], f.loudness);
            return st != FT_OK ? st : ft_fail(ctx, FT_ERR_ARG, fn + ": item " + std::to_string(bad.item) + ": a bad chain");
        }
    } else {
        FT_TRY(fx_refuse(ctx, fn, sample_rate, fx->speed_pct, fx->pitch_cents, &d[0], fx->loudness));
    }
    FT_TRY(codec_ready(ctx));
    if (!codes || !audio || !total || !cuts || B < 1 || B > JOIN_MAX_ITEMS || T < 1) return ft_fail(ctx, FT_ERR_ARG, fn + ": bad argument");
    if (T > ctx->cc.max_frames) return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": T exceeds max_frames");
    if (!per_item) std::fill(d + 1, d + B, d[0]);
    CodecState* s = ctx->codec;
    const int R = ctx->cc.n_codebooks + 1;
    int64_t n[JOIN_MAX_ITEMS], off[JOIN_MAX_ITEMS], frames = 0, need = 0;
    if (const char* why = item_fx_lens(d, B, T, lens, s->frame_len, n, &frames)) return ft_fail(ctx, FT_ERR_ARG, fn + ": " + why);
    if (frames > ctx->cc.max_frames) return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": sum(lens) exceeds max_frames");
    if (const char* why = join_check(B, n, jp, gaps, started, capacity, &need)) return ft_fail(ctx, FT_ERR_ARG, fn + ": " + why);
    const int64_t in_floats = join_offsets(B, n, off);
    const ItemFxUnion u = item_fx_union(d, B, n);
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_TRY(fx_prepare(ctx, d, u.hops, B));
    FT_TRY(join_alloc(ctx, (size_t)in_floats, (size_t)need));
    // the items as decode_items runs them (one synchronize each, as there), their samples left side by side in join_in
    for (int b = 0; b < B; ++b) {
        const int Tb = lens ? lens[b] : T;
        if (Tb == 0) continue;
        Fx g;
        const bool staged = item_stages(s, d[b], (long long)Tb * s->frame_len, g);
        FT_TRY(decode_one(ctx, codes + (size_t)b * R * T, T, Tb, s->join_in + off[b], nullptr, staged ? &g : nullptr, hipMemcpyDeviceToDevice));
    }
    if (u.levelled > 0) {       // the levelled items alone, each toward its own target
        float* x[JOIN_MAX_ITEMS];
        int64_t nl[JOIN_MAX_ITEMS];
        int targets[JOIN_MAX_ITEMS];
        for (int k = 0; k < u.levelled; ++k) {
            x[k] = s->join_in + off[u.lv[k]];
            nl[k] = n[u.lv[k]];
            targets[k] = d[u.lv[k]].level;
        }
        FT_TRY(level_enqueue(ctx, u.levelled, x, nl, d[0].rate, targets));
    }
    FT_TRY(join_run(ctx, B, n, off, jp, gaps, started, audio, total, cuts, need, false));
    if (per_item && infos) {
        const ft_level_info none = {-INFINITY, 0.f, 1.f, 0, 0, 0};
        for (int b = 0; b < B; ++b) {
            memset(&infos[b], 0, sizeof(ft_level_info));
            infos[b] = none;
        }
    }
    if (u.levelled > 0) level_fetch(s, u.levelled, infos, u.lv);
    return FT_OK;
}

extern "C" ft_status ft_codec_decode_join(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                          int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents, const ft_join_params* jp,
                                          const int64_t* gaps, int32_t started, float* audio, int64_t capacity, int64_t* total,
                                          int64_t* cuts) {
    const ft_item_fx fx = {speed_pct, pitch_cents, 0};
    return decode_join(ctx, "ft_codec_decode_join", codes, B, T, lens, sample_rate, &fx, false, jp, gaps, started, audio, capacity,
                       total, cuts, nullptr);
}

extern "C" ft_status ft_codec_decode_join_level(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                                int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents, int32_t loudness,
                                                const ft_join_params* jp, const int64_t* gaps, int32_t started, float* audio,
                                                int64_t capacity, int64_t* total, int64_t* cuts, ft_level_info* infos) {
    const ft_item_fx fx = {speed_pct, pitch_cents, loudness};
    return decode_join(ctx, "ft_codec_decode_join_level", codes, B, T, lens, sample_rate, &fx, false, jp, gaps, started, audio,
                       capacity, total, cuts, infos);
}

extern "C" ft_status ft_codec_decode_join_items(ft_ctx* ctx, const int32_t* codes, int32_t B, int32_t T, const int32_t* lens,
                                                int32_t sample_rate, const ft_item_fx* fx, const ft_join_params* jp,
                                                const int64_t* gaps, int32_t started, float* audio, int64_t capacity,
                                                int64_t* total, int64_t* cuts, ft_level_info* infos) {
    return decode_join(ctx, "ft_codec_decode_join_items", codes, B, T, lens, sample_rate, fx, true, jp, gaps, started, audio,
                       capacity, total, cuts, infos);
}

extern "C" ft_status ft_test_join(ft_ctx* ctx, const float* x, int32_t B, int64_t stride, const int64_t* n, const ft_join_params* jp,
                                  const int64_t* gaps, int32_t started, float* y, int64_t capacity, int64_t* total, int64_t* cuts) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!x || !y || !total || !cuts || stride < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_join: bad argument");
    int64_t need = 0, off[JOIN_MAX_ITEMS];
    if (const char* why = join_check(B, n, jp, gaps, started, capacity, &need)) return ft_fail(ctx, FT_ERR_ARG, std::string("ft_test_join: ") + why);
    for (int b = 0; b < B; ++b)
        if (n[b] > stride) return ft_fail(ctx, FT_ERR_ARG, "ft_test_join: an item longer than the stride");
    const int64_t in_floats = join_offsets(B, n, off);
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_TRY(join_alloc(ctx, (size_t)in_floats, (size_t)need));
    for (int b = 0; b < B; ++b)
        if (n[b] > 0)
            FT_HIP(ctx, hipMemcpyAsync(s->join_in + off[b], x + (size_t)b * stride, (size_t)n[b] * sizeof(float), hipMemcpyHostToDevice, s->stream));
    FT_TRY(join_run(ctx, B, n, off, jp, gaps, started, y, total, cuts, need, true));
    const uint32_t mark = 0xFFFFFFFEu;
    for (int64_t i = need; i < capacity; ++i) memcpy(y + i, &mark, sizeof mark);
    return FT_OK;
}

// Hops (and nodes) of the longest waveform a stream or ft_codec_ride can see at `rate`: max_frames frames at speed 0.5.
static size_t rd_max_hops(ft_ctx* ctx, int rate) {
    const long long most = (2LL * ctx->cc.max_frames * ctx->codec->frame_len * rate + RS_FI - 1) / RS_FI;
    return (size_t)(most / chain::lv_hop(rate)) + 4;
}

static ft_status stream_begin_fx(ft_ctx* ctx, const std::string& fn, int32_t sample_rate, int32_t pct, ft_codec_stream** out,
                                 int32_t cents = 0, int32_t live = 0) {
    if (!ctx || !out) return FT_ERR_ARG;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, fn, sample_rate, pct, cents, &d, 0, live));
    FT_TRY(codec_ready(ctx));
    CodecState* s = ctx->codec;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        FT_HIP(ctx, hipSetDevice(ctx->device));
        FT_TRY(fx_prepare(ctx, &d));
    }
    ft_codec_stream* sc = nullptr;
    FT_TRY(ft_codec_stream_begin(ctx, &sc));
    if (!d.any()) {
        *out = sc;
        return FT_OK;
    }
    StageChain c = d.fresh();
    bool ok = true;   // (as ft_codec_stream_begin: the stream is not visible to other calls yet)
    auto zalloc = [&](float** q, size_t n) {
        void* v = nullptr;
        ok = ok && hipMalloc(&v, n * sizeof(float)) == hipSuccess;
        if (!ok) return;
        sc->owned.push_back(v);
        *q = (float*)v;
        ok = hipMemsetAsync(v, 0, n * sizeof(float), s->stream) == hipSuccess;   // the input before the first sample
    };
    for (int k = 0; k < 2 && c.rs.tab; ++k) zalloc(&c.rs.carry[k], (size_t)c.rs.tab->K);
    for (int k = 0; k < 2 && c.ts.on; ++k) {
        zalloc(&c.ts.carry[k], (size_t)TS_CARRY);
        zalloc(&c.ts.state[k], (size_t)TS_STATE);
    }
    for (int k = 0; k < 2 && c.ps.tab; ++k) zalloc(&c.ps.carry[k], (size_t)c.ps.tab->K);
    if (c.rd.target != 0) {   // the ride stage: two carries, and a hop sum, a peak, a v and a node per hop of the longest stream
        const size_t hops = rd_max_hops(ctx, d.rate);
        float *e = nullptr, *v = nullptr;
        for (int k = 0; k < 2; ++k) zalloc(&c.rd.carry[k], (size_t)(chain::RD_A + 1) * c.rd.H);
        zalloc(&e, 2 * hops);
        zalloc(&v, 2 * hops);
        zalloc(&c.rd.p, hops);
        zalloc(&c.rd.g, hops);
        c.rd.e = (double*)e;
        c.rd.v = (double*)v;
    }
    ok = ok && hipStreamSynchronize(s->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ft_codec_stream_end(ctx, sc);
        return ft_fail(ctx, FT_ERR_NOMEM, fn + ": could not set up the output stages' carry");
    }
    sc->fx = c;
    *out = sc;
    return FT_OK;
}

extern "C" ft_status ft_codec_stream_begin_at(ft_ctx* ctx, int32_t sample_rate, ft_codec_stream** out) {
    return stream_begin_fx(ctx, "ft_codec_stream_begin_at", sample_rate, 100, out);
}

extern "C" ft_status ft_codec_stream_begin_fx(ft_ctx* ctx, int32_t sample_rate, int32_t speed_pct, ft_codec_stream** out) {
    return stream_begin_fx(ctx, "ft_codec_stream_begin_fx", sample_rate, speed_pct, out);
}

extern "C" ft_status ft_codec_stream_begin_fxp(ft_ctx* ctx, int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents,
                                               ft_codec_stream** out) {
    return stream_begin_fx(ctx, "ft_codec_stream_begin_fxp", sample_rate, speed_pct, out, pitch_cents);
}

extern "C" ft_status ft_codec_stream_begin_live(ft_ctx* ctx, int32_t sample_rate, int32_t speed_pct, int32_t pitch_cents,
                                                int32_t live, ft_codec_stream** out) {
    return stream_begin_fx(ctx, live != 0 ? "ft_codec_stream_begin_live" : "ft_codec_stream_begin_fxp", sample_rate, speed_pct, out,
                           pitch_cents, live);
}

extern "C" ft_status ft_codec_stream_decode_many_at(ft_ctx* ctx, int32_t n, ft_codec_stream* const* streams, const int32_t* codes,
                                                    const int32_t* lens, const int32_t* final, float* audio, int64_t* out_lens) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (n < 1 || !streams || !codes || !lens || !audio || !out_lens)
        return ft_fail(ctx, FT_ERR_ARG, "ft_codec_stream_decode_many_at: bad argument");
    FT_TRY(many_check(ctx, "ft_codec_stream_decode_many_at", n, streams, lens, final, true));
    CodecState* s = ctx->codec;
    const int fl = s->frame_len;
    // what every stream's stages take and emit in this call, walked in chain order (fx_chain.h)
    long long total_out = 0, total_ts = 0, total_ps = 0, total_rd = 0;
    bool any_fx = false, ride = false;
    std::vector<ChainPlan> plan(n);
    for (int j = 0; j < n; ++j) {
        const StageChain& c = streams[j]->fx;
        plan[j] = c.plan((long long)lens[j] * fl, final && final[j]);
        if (c.ts.held(plan[j].ts) > TS_CARRY) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_stream_decode_many_at: time-scale carry out of step");
        if (c.ts.on) total_ts += plan[j].ts.out;
        if (c.ps.tab) total_ps += plan[j].ps.out;
        if (c.rd.held(plan[j].rd) >= (long long)(chain::RD_A + 1) * c.rd.H || (size_t)plan[j].rd.nodes > (c.rd.target != 0 ? rd_max_hops(ctx, c.rd.rate) : 1))
            return ft_fail(ctx, FT_ERR_STATE, "ft_codec_stream_decode_many_at: ride carry out of step");
        total_out += plan[j].rs.out;
        total_rd += plan[j].rd.out;
        any_fx = any_fx || c.any();
        ride = ride || c.rd.target != 0;
    }
    if (any_fx && ((size_t)total_out > s->rs_cap || (size_t)total_ts > s->ts_cap || (size_t)total_ps > s->ts_cap ||
                   (ride && (size_t)total_rd > s->rd_cap)))
        return ft_fail(ctx, FT_ERR_TOO_LONG, "ft_codec_stream_decode_many_at: output buffer");
    // the codec runs over the streams with frames (their code blocks are back to back, as the call's)
    std::vector<ft_codec_stream*> cs;
    std::vector<int32_t> cl;
    for (int j = 0; j < n; ++j)
        if (lens[j] > 0) { cs.push_back(streams[j]); cl.push_back(lens[j]); }
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    TraceScope untraced(s, false);   // the launch trace covers ft_codec_stream_decode_many only: an armed trace is dropped here
    if (!any_fx) {   // the codec's rate and pace only: ft_codec_stream_decode_many
        if (!cs.empty()) FT_TRY(decode_many(ctx, (int)cs.size(), cs.data(), codes, cl.data(), audio));
        for (int j = 0; j < n; ++j) out_lens[j] = plan[j].rd.out;
        return FT_OK;
    }
    Fx fx;
    long long P = 0;
    for (int j = 0; j < n; ++j) {
        chain_segs(streams[j]->fx, plan[j], s->audio + P * fl, j, nullptr, fx, ride);
        P += lens[j];
    }
    if (!cs.empty()) {
        FT_TRY(decode_many(ctx, (int)cs.size(), cs.data(), codes, cl.data(), audio, &fx));
    } else {   // tails only
        FT_TRY(call_tail(ctx, &fx, audio, 0, "output stage launch: "));
    }
    for (int j = 0; j < n; ++j) {
        ft_codec_stream* sc = streams[j];
        out_lens[j] = plan[j].rd.out;
        if (!sc->fx.any()) continue;
        sc->fx.commit(plan[j]);
        sc->finished = final && final[j];
    }
    return FT_OK;
}

// ---- ride stage alone (fishtts_hip.h: ft_ride_plan, ft_codec_ride; fishtts_hip_test.h: ft_test_ride_streams)
extern "C" ft_status ft_ride_plan(int32_t sample_rate, int64_t n_in, int32_t final, int64_t* nodes, int64_t* n_out) {
    int l = 1, m = 1, k = 0;
    if (n_in < 0 || chain::rs_design(sample_rate, &l, &m, &k, nullptr)) return FT_ERR_ARG;
    const chain::RdPlan p = chain::rd_plan(chain::lv_hop(sample_rate), n_in, final != 0);
    if (nodes) *nodes = p.nodes;
    if (n_out) *n_out = p.out;
    return FT_OK;
}

// What the launches of a ride call left behind, after the call's one synchronize.
static ft_status rd_finish(ft_ctx* ctx) {
    FT_HIP(ctx, hipStreamSynchronize(ctx->codec->stream));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("ride launch: ") + hipGetErrorString(e));
    return FT_OK;
}

extern "C" ft_status ft_codec_ride(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, int32_t target, float* y,
                                   float* nodes) {
    const std::string fn = "ft_codec_ride";
    if (!ctx) return FT_ERR_ARG;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, fn, sample_rate, 100, 0, &d, 0, target));
    FT_TRY(codec_ready(ctx));
    if ((!x && n > 0) || !y || n < 0) return ft_fail(ctx, FT_ERR_ARG, fn + ": bad argument");
    CodecState* s = ctx->codec;
    const int64_t most = (2 * (int64_t)ctx->cc.max_frames * s->frame_len * RS_MAX_RATE + RS_FI - 1) / RS_FI;
    if (n > most) return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": longer than the longest item a decode gives");
    chain::RdStage r = d.fresh().rd;
    const size_t nn = (size_t)((n + r.H - 1) / r.H) + 1;
    if (target == 0) {   // no stage
        if (n > 0) memcpy(y, x, (size_t)n * sizeof(float));
        for (size_t k = 0; nodes && k < nn; ++k) nodes[k] = 1.f;
        return FT_OK;
    }
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_TRY(rd_alloc(ctx, (size_t)std::max(n, (int64_t)4)));
    FT_TRY(cgrow(ctx, &s->lv_x, &s->lv_xcap, (size_t)std::max(n, (int64_t)4)));
    FT_TRY(cgrow(ctx, &s->rd_e, &s->rd_ecap, nn));
    FT_TRY(cgrow(ctx, &s->rd_v, &s->rd_vcap, nn));
    FT_TRY(cgrow(ctx, &s->rd_p, &s->rd_pcap, nn));
    FT_TRY(cgrow(ctx, &s->rd_g, &s->rd_gcap, nn));
    r.e = s->rd_e; r.v = s->rd_v; r.p = s->rd_p; r.g = s->rd_g;
    if (n > 0) FT_HIP(ctx, hipMemcpyAsync(s->lv_x, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    Fx fx;
    fx.rd.push_back(rd_seg_of(r, r.plan(n, true), s->lv_x));     // a stream whose one call is its last: nothing carried in or out
    FT_TRY(rd_enqueue(ctx, fx, y));
    if (nodes) FT_HIP(ctx, hipMemcpyAsync(nodes, s->rd_g, nn * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    return rd_finish(ctx);
}

extern "C" ft_status ft_test_ride_streams(ft_ctx* ctx, const float* x, int32_t B, int64_t stride, const int64_t* n, int32_t sample_rate,
                                          int32_t target, const int64_t* cuts, int32_t ncuts, float* y, float* nodes, int64_t* emitted) {
    const std::string fn = "ft_test_ride_streams";
    if (!ctx) return FT_ERR_ARG;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, fn, sample_rate, 100, 0, &d, 0, target));
    FT_TRY(codec_ready(ctx));
    if (!x || !n || !y || !nodes || !emitted || B < 1 || B > RS_MAX_SEGS || stride < 1 || ncuts < 0 || (ncuts > 0 && !cuts) || target == 0)
        return ft_fail(ctx, FT_ERR_ARG, fn + ": bad argument");
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        if (n[b] < 0 || n[b] > stride) return ft_fail(ctx, FT_ERR_ARG, fn + ": a waveform longer than the stride");
        total += n[b];
    }
    for (int j = 0; j < ncuts; ++j)
        if (cuts[j] < (j ? cuts[j - 1] : 0)) return ft_fail(ctx, FT_ERR_ARG, fn + ": cuts must not descend");
    CodecState* s = ctx->codec;
    const int H = chain::lv_hop(sample_rate);
    const size_t nn = (size_t)(stride / H) + 2;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_TRY(rd_alloc(ctx, (size_t)std::max(total, (int64_t)4)));
    FT_TRY(cgrow(ctx, &s->lv_x, &s->lv_xcap, (size_t)std::max(total, (int64_t)4)));
    // the streams' state in one allocation, freed when the call ends: per stream two carries, e, v, p, g
    const size_t held = (size_t)(chain::RD_A + 1) * H, per = 2 * held + 6 * nn;
    float* blk = nullptr;
    if (hipMalloc((void**)&blk, (size_t)B * per * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return ft_fail(ctx, FT_ERR_NOMEM, fn + ": the streams' state");
    }
    struct Free { float* p; ~Free() { hipFree(p); } } guard{blk};
    FT_HIP(ctx, hipMemsetAsync(blk, 0, (size_t)B * per * sizeof(float), s->stream));
    std::vector<chain::RdStage> st((size_t)B, d.fresh().rd);
    for (int b = 0; b < B; ++b) {
        float* q = blk + (size_t)b * per;
        st[b].e = (double*)q;
        st[b].v = (double*)(q + 2 * nn);
        st[b].p = q + 4 * nn;
        st[b].g = q + 5 * nn;
        st[b].carry[0] = q + 6 * nn;
        st[b].carry[1] = q + 6 * nn + held;
    }
    std::vector<float> got((size_t)std::max(total, (int64_t)1));
    for (int j = 0; j <= ncuts; ++j) {
        const bool fin = j == ncuts;
        Fx fx;
        std::vector<chain::RdPlan> plan((size_t)B);
        int64_t off = 0;
        for (int b = 0; b < B; ++b) {
            const int64_t lo = std::min(n[b], j ? cuts[j - 1] : 0), hi = fin ? n[b] : std::min(n[b], cuts[j]);
            if (hi > lo)
                FT_HIP(ctx, hipMemcpyAsync(s->lv_x + off, x + (size_t)b * stride + lo, (size_t)(hi - lo) * sizeof(float), hipMemcpyHostToDevice, s->stream));
            plan[b] = st[b].plan(hi - lo, fin);
            if (st[b].held(plan[b]) >= (long long)held) return ft_fail(ctx, FT_ERR_STATE, fn + ": ride carry out of step");
            fx.rd.push_back(rd_seg_of(st[b], plan[b], s->lv_x + off));
            off += hi - lo;
        }
        FT_TRY(rd_enqueue(ctx, fx, got.data()));
        FT_TRY(rd_finish(ctx));
        off = 0;
        for (int b = 0; b < B; ++b) {
            memcpy(y + (size_t)b * stride + st[b].nout, got.data() + off, (size_t)plan[b].out * sizeof(float));
            off += plan[b].out;
            emitted[(size_t)j * B + b] = plan[b].out;
            st[b].commit(plan[b]);
        }
    }
    for (int b = 0; b < B; ++b)
        FT_HIP(ctx, hipMemcpy(nodes + (size_t)b * nn, st[b].g, (size_t)st[b].nodes * sizeof(float), hipMemcpyDeviceToHost));
    return FT_OK;
}

extern "C" ft_status ft_test_resample(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, float* y, int64_t* n_out) {
    if (!ctx) return FT_ERR_ARG;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, "ft_test_resample", sample_rate, 100, 0, &d));
    FT_TRY(codec_ready(ctx));
    if (!x || !y || !n_out || n < 1) return ft_fail(ctx, FT_ERR_ARG, "ft_test_resample: bad argument");
    CodecState* s = ctx->codec;
    if (n > (int64_t)ctx->cc.max_frames * s->frame_len) return ft_fail(ctx, FT_ERR_TOO_LONG, "ft_test_resample: longer than max_frames of audio");
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_TRY(fx_prepare(ctx, &d));
    *n_out = d.out_len(n);
    Fx g;
    if (!item_stages(s, d, n, g)) {
        memcpy(y, x, (size_t)n * sizeof(float));
        return FT_OK;
    }
    FT_HIP(ctx, hipMemcpyAsync(s->audio, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    return call_tail(ctx, &g, y, 0, "resample launch: ");
}

extern "C" ft_status ft_test_timescale(ft_ctx* ctx, const float* x, int64_t n, int32_t speed_pct, float* y, int64_t* n_out,
                                       int32_t* deltas, int32_t* n_frames) {
    if (!ctx) return FT_ERR_ARG;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, "ft_test_timescale", RS_FI, speed_pct, 0, &d));
    FT_TRY(codec_ready(ctx));
    if (!x || !y || !n_out || n < 1) return ft_fail(ctx, FT_ERR_ARG, "ft_test_timescale: bad argument");
    CodecState* s = ctx->codec;
    if (n > (int64_t)ctx->cc.max_frames * s->frame_len) return ft_fail(ctx, FT_ERR_TOO_LONG, "ft_test_timescale: longer than max_frames of audio");
    StageChain c = d.fresh();
    c.ts.on = true;   // the hook runs the stage at 100 percent too
    const ChainPlan p = c.plan(n, true);
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_TRY(ts_alloc(ctx));
    *n_out = p.ts.out;
    if (n_frames) *n_frames = p.ts.k1;
    FT_HIP(ctx, hipMemcpyAsync(s->audio, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    Fx g;
    chain_segs(c, p, s->audio, 0, s->ts_delta, g);
    FT_TRY(call_tail(ctx, &g, y, 0, "time-scale launch: "));
    if (deltas) FT_HIP(ctx, hipMemcpy(deltas, s->ts_delta, (size_t)p.ts.k1 * sizeof(int), hipMemcpyDeviceToHost));
    return FT_OK;
}

extern "C" ft_status ft_test_pitch(ft_ctx* ctx, const float* x, int64_t n, int32_t speed_pct, int32_t cents, float* y, int64_t* n_out,
                                   float* mid, int64_t* n_mid, int32_t* deltas, int32_t* n_frames) {
    if (!ctx) return FT_ERR_ARG;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, "ft_test_pitch", RS_FI, speed_pct, cents, &d));
    FT_TRY(codec_ready(ctx));
    if (!x || !y || !n_out || n < 1 || cents == 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_pitch: bad argument");
    CodecState* s = ctx->codec;
    if (n > (int64_t)ctx->cc.max_frames * s->frame_len) return ft_fail(ctx, FT_ERR_TOO_LONG, "ft_test_pitch: longer than max_frames of audio");
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    FT_TRY(fx_prepare(ctx, &d));
    const StageChain c = d.fresh();
    const ChainPlan p = c.plan(n, true);
    *n_out = p.ps.out;
    if (n_mid) *n_mid = p.ts.out;
    if (n_frames) *n_frames = p.ts.k1;
    FT_HIP(ctx, hipMemcpyAsync(s->audio, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    Fx g;
    chain_segs(c, p, s->audio, 0, s->ts_delta, g);
    FT_TRY(call_tail(ctx, &g, y, 0, "pitch launch: "));
    if (mid) FT_HIP(ctx, hipMemcpy(mid, c.ts.on ? s->ts_out : s->audio, (size_t)p.ts.out * sizeof(float), hipMemcpyDeviceToHost));
    if (deltas && p.ts.k1 > 0) FT_HIP(ctx, hipMemcpy(deltas, s->ts_delta, (size_t)p.ts.k1 * sizeof(int), hipMemcpyDeviceToHost));
    return FT_OK;
}

static ft_status rvq_search(ft_ctx* ctx, hipStream_t st, const float* z, int T, int* codes_dev) {
    const ft_codec_config& c = ctx->cc;
    CodecState* s = ctx->codec;
    RvqEncP rp{z, s->inw, s->inb, s->cbn, s->cn2, s->tables, c.n_codebooks + 1, c.semantic_codebook_size, c.codebook_size,
               c.latent_dim, c.codebook_dim, T, codes_dev};
    rvq_encode_kernel<<<T, 256, (size_t)c.latent_dim * sizeof(float), st>>>(rp);
    return FT_OK;
}

extern "C" ft_status ft_codec_rvq_encode(ft_ctx* ctx, const float* z, int32_t T, int32_t* codes) {
    if (!ctx) return FT_ERR_ARG;
    if (!ctx->has_codec || !ctx->codec || !ctx->codec->has_enc) return ft_fail(ctx, FT_ERR_STATE, "codec encoder not configured");
    FT_TRY(codec_ready(ctx));
    const ft_codec_config& c = ctx->cc;
    if (!z || !codes || T < 1 || T > c.max_enc_frames) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_rvq_encode: bad argument");
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    const int R = c.n_codebooks + 1;
    FT_HIP(ctx, hipMemcpyAsync(s->enc_zq, z, (size_t)T * c.latent_dim * sizeof(float), hipMemcpyHostToDevice, s->stream));
    FT_TRY(rvq_search(ctx, s->stream, s->enc_zq, T, s->enc_codes));
    FT_HIP(ctx, hipMemcpyAsync(codes, s->enc_codes, (size_t)R * T * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    FT_HIP(ctx, hipStreamSynchronize(s->stream));
    return FT_OK;
}

// The encoder over n_samples samples at `audio` (host or device: `src_kind`), enqueued on the codec's stream: the zero fill to
// whole frames, the copy into enc_audio, the chain, the quantiser search, and the copy of the (n_codebooks+1) x T' codes to
// `codes` (host or device: `dst_kind`).  The caller holds s->mu, has checked 1 <= n_samples <= max_enc_frames frames, and
// synchronizes.
static ft_status encode_enqueue(ft_ctx* ctx, const float* audio, hipMemcpyKind src_kind, int64_t n_samples, int* codes,
                                hipMemcpyKind dst_kind) {
    CodecState* s = ctx->codec;
    const ft_codec_config& c = ctx->cc;
    const long fl = s->enc_frame_len;
    const long Tf = (n_samples + fl - 1) / fl;
    const long T0 = Tf * fl;
    hipStream_t st = s->stream;
    const int D = c.latent_dim, H = c.tf_n_head, hd = c.tf_head_dim, R = c.n_codebooks + 1;
    FT_HIP(ctx, hipMemsetAsync(s->enc_audio, 0, (size_t)T0 * sizeof(float), st));
    FT_HIP(ctx, hipMemcpyAsync(s->enc_audio, audio, (size_t)n_samples * sizeof(float), src_kind, st));
    // Encoder (vocoder.py:539-575).  r = raw residual stream, a = Snake'd operand of the next conv, hs = inner buffer
    bf16_t *r = s->ebuf[0], *a = s->ebuf[1], *hs = s->ebuf[2], *o = s->ebuf[3];
    long T = T0;
    {
        EncInP ep{s->enc_audio, s->enc_w0, s->enc_b0, s->enc[0].u[0].a0, T, c.encoder_dim, r, a};
        enc_conv_in_kernel<<<gridfor(T * c.encoder_dim), 256, 0, st>>>(ep);
        if (s->trace) trace_rec(s, st, "enc.in", T, c.encoder_dim, -1, 6, 7, 1, {{0, r, 0}, {1, a, 0}});
    }
    for (size_t bi = 0; bi < s->enc.size(); ++bi) {
        const CodecState::EncBlock& b = s->enc[bi];
        for (int ui = 0; ui < 3; ++ui) {
            const CodecState::EncUnit& ru = b.u[ui];
            { GemmIO io{a, b.cin, (int)T, (int)T}; io.out_act = hs; io.alpha = ru.a2; io.ldo = b.cin; gemm_t(s, st, ru.c7, io, "%senc.%d.u%d.c7", (int)bi, ui); }
            const float* next_alpha = ui < 2 ? b.u[ui + 1].a0 : b.a3;
            { GemmIO io{hs, b.cin, (int)T, (int)T}; io.resid_bf = r; io.ldr = b.cin; io.out_bf = ui < 2 ? r : nullptr;
              io.out_act = a; io.alpha = next_alpha; io.ldo = b.cin; gemm_t(s, st, ru.c1, io, "%senc.%d.u%d.c1", (int)bi, ui); }
        }
        // strided conv on the [T/s][s*cin] view of a; raw output to o (no transformer) or to the f32 stream
        const long Tn = T / b.s;
        const bool has_tf = !b.tf.empty();
        { GemmIO io{a, (long)b.s * b.cin, (int)Tn, (int)Tn}; if (has_tf) io.out_f32 = s->enc_x; else io.out_bf = o; io.ldo = b.cout; gemm_t(s, st, b.sc, io, "%senc.%d.sc", (int)bi); }
        T = Tn;
        if (has_tf)
            run_transformer(ctx, Layout::plain((int)T, s->e_qkv), b.tf, b.tf_norm, s->enc_x, b.cout, b.cout / 64, 64, 3 * b.cout,
                            c.enc_tf_window, s->rope_enc, s->e_xn, s->e_y, s->e_g, o, nullptr, tname("enc.%d.tf.", (int)bi).c_str());
        const float* alpha_next = bi + 1 < s->enc.size() ? s->enc[bi + 1].u[0].a0 : s->enc_a_last;
        snake_bf_rows_kernel<<<gridfor(T * b.cout), 256, 0, st>>>(o, alpha_next, a, T * b.cout, b.cout);
        if (s->trace) trace_rec(s, st, tname("enc.%d.snake", (int)bi), T, b.cout, -1, 0, 0, 0, {{1, a, 0}});
        std::swap(r, o);  // the raw output is the next block's residual stream
    }
    bf16_t* z = hs;   // [T][D]
    { GemmIO io{a, s->enc[s->enc.size() - 1].cout, (int)T, (int)T}; io.out_bf = z; io.ldo = D; gemm_t(s, st, s->enc_out, io, "%senc.out"); }
    // quantizer.downsample (vocoder.py:724-735): strided conv k = s = 2, ConvNeXt
    bf16_t *u = r, *n = a, *h = o;
    for (size_t j = 0; j < s->down.size(); ++j) {
        const UpStage& ds = s->down[j];
        const long Tn = T / ds.f;
        { GemmIO io{z, (long)ds.f * D, (int)Tn, (int)Tn}; io.out_bf = u; io.ldo = D; gemm_t(s, st, ds.ct, io, "%sdown.%d.sc", (int)j); }
        T = Tn;
        dwconv_ln_kernel<<<(int)T, 256, D * sizeof(float), st>>>(DwLnP{u, ds.dw_w, ds.dw_b, ds.ln_w, ds.ln_b, (int)T, D, n});
        if (s->trace) trace_rec(s, st, tname("down.%d.dwln", (int)j), T, D, -1, 6, 7, 0, {{0, n, 0}});
        { GemmIO io{n, D, (int)T, (int)T}; io.act = ACT_GELU; io.out_bf = h; io.ldo = 4 * D; gemm_t(s, st, ds.pw1, io, "%sdown.%d.pw1", (int)j); }
        const bool last = j + 1 == s->down.size();
        { GemmIO io{h, 4 * D, (int)T, (int)T}; io.gamma = ds.gamma; io.resid_bf = u; io.ldr = D; io.out_bf = z; io.ldo = D;
          if (last) io.out_f32 = s->enc_x; gemm_t(s, st, ds.pw2, io, "%sdown.%d.pw2", (int)j); }
    }
    if (s->down.empty()) {
        bf16_rows_to_f32_kernel<<<gridfor(T * D), 256, 0, st>>>(z, s->enc_x, T * D);
        if (s->trace) trace_rec(s, st, "down.f32", T, D, -1, 0, 0, 0, {{2, s->enc_x, 1}});
    }
    if (T != Tf) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_encode: stage rates do not multiply to the frame length");
    // pre_module (window-limited transformer), then the residual quantiser search
    run_transformer(ctx, Layout::plain((int)T, s->e_qkv), s->pre, s->pre_norm, s->enc_x, D, H, hd, c.tf_ffn, c.tf_window, s->rope,
                    s->e_xn, s->e_y, s->e_g, nullptr, s->enc_zq, "pre.");
    FT_TRY(rvq_search(ctx, st, s->enc_zq, (int)T, s->enc_codes));
    FT_HIP(ctx, hipMemcpyAsync(codes, s->enc_codes, (size_t)R * T * sizeof(int), dst_kind, st));
    return FT_OK;
}

extern "C" ft_status ft_codec_encode(ft_ctx* ctx, const float* audio, int64_t n_samples, int32_t* codes, int32_t* out_frames) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx, false));
    CodecState* s = ctx->codec;
    if (!s->has_enc) return ft_fail(ctx, FT_ERR_STATE, "codec encoder not configured (encoder_dim = 0)");
    FT_TRY(codec_ready(ctx));
    if (!audio || !codes || !out_frames || n_samples < 1) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_encode: bad argument");
    const ft_codec_config& c = ctx->cc;
    const long fl = s->enc_frame_len;
    const long Tf = (n_samples + fl - 1) / fl;            // code frames (vocoder.py:891-892, 903)
    if (Tf > c.max_enc_frames) return ft_fail(ctx, FT_ERR_TOO_LONG, "ft_codec_encode: audio longer than max_enc_frames");
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    TraceScope traced(s, true);
    hipStream_t st = s->stream;
    FT_TRY(encode_enqueue(ctx, audio, hipMemcpyHostToDevice, n_samples, codes, hipMemcpyDeviceToHost));
    FT_HIP(ctx, hipStreamSynchronize(st));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("codec encode launch: ") + hipGetErrorString(e));
    *out_frames = (int32_t)Tf;
    return FT_OK;
}

extern "C" int32_t ft_codec_enc_frame_len(const ft_ctx* ctx) { return ctx && ctx->codec ? ctx->codec->enc_frame_len : 0; }

extern "C" int32_t ft_codec_frame_len(const ft_ctx* ctx) { return ctx && ctx->codec ? ctx->codec->frame_len : 0; }

// ---- reference intake (fishtts_hip.h: ft_intake_filter .. ft_codec_encode_items; IntakeSeg and intake_kernel in
// stage_kernels.h, the filter design in fx_chain.h)
static_assert(sizeof(ft_intake_info) == 80 && offsetof(ft_intake_info, level) == 48, "ft_intake_info layout");
constexpr int64_t IN_MAX_RAW = (int64_t)1 << 30;

extern "C" ft_status ft_intake_filter(int32_t rate_in, int32_t* L, int32_t* M, int32_t* K, float* table) {
    int l = 1, m = 1, k = 0;
    std::vector<float> w;
    if (chain::rs_design_in(rate_in, &l, &m, &k, table ? &w : nullptr)) return FT_ERR_ARG;
    if (L) *L = l;
    if (M) *M = m;
    if (K) *K = k;
    if (table && !w.empty()) memcpy(table, w.data(), w.size() * sizeof(float));
    return FT_OK;
}

extern "C" int64_t ft_intake_len(int32_t rate_in, int64_t n) {
    int l = 1, m = 1, k = 0;
    if (n < 0 || chain::rs_design_in(rate_in, &l, &m, &k, nullptr)) return -1;
    return (n * l + m - 1) / m;
}

// The device table of input rate `rate` (uploaded on its first use); the caller holds s->mu.
static ft_status in_table(ft_ctx* ctx, int rate, const CodecState::RsTab** out) {
    CodecState* s = ctx->codec;
    auto it = s->in_tabs.find(rate);
    if (it == s->in_tabs.end()) {
        CodecState::RsTab t;
        std::vector<float> w;
        if (const char* e = chain::rs_design_in(rate, &t.L, &t.M, &t.K, &w)) return ft_fail(ctx, FT_ERR_ARG, e);
        if (t.K > 0) {
            FT_TRY(cmalloc(ctx, &t.w, w.size()));
            FT_TRY(cupload(ctx, t.w, w.data(), w.size() * sizeof(float)));
        }
        it = s->in_tabs.emplace(rate, t).first;
    }
    *out = &it->second;
    return FT_OK;
}

// Both entry points: every check, then raw bytes -> intake -> level -> join on the codec's stream; `enc`: the encoder over
// the kept pieces and their codes to `codes`, else the pieces themselves to `audio`.  `held`: the caller holds s->mu and
// wants the pieces left in join_out for a stage of its own (the mix stage's bed); `audio` is not written.
static ft_status intake_run(ft_ctx* ctx, const std::string& fn, int32_t B, const ft_intake_item* items, const ft_join_params* jp,
                            int32_t loudness, bool enc, float* audio, int32_t* codes, int64_t capacity, int64_t* lens, ft_intake_info* infos,
                            bool held = false) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx, false));
    CodecState* s = ctx->codec;
    if (enc && !s->has_enc) return ft_fail(ctx, FT_ERR_STATE, fn + ": codec encoder not configured (encoder_dim = 0)");
    FT_TRY(codec_ready(ctx));
    if (!items || !jp || !infos || (enc ? !codes : ((!audio && !held) || !lens)) || B < 1 || B > JOIN_MAX_ITEMS)
        return ft_fail(ctx, FT_ERR_ARG, fn + ": bad argument (null pointer, or B outside [1, 64])");
    if (!chain::lv_ok(loudness))
        return ft_fail(ctx, FT_ERR_ARG, fn + ": loudness outside [-5000, -500] hundredths of a LUFS (" + std::to_string(loudness) + ")");
    const int64_t fl = s->has_enc ? s->enc_frame_len : 0;
    const int64_t most = (2 * (int64_t)ctx->cc.max_frames * s->frame_len * RS_MAX_RATE + RS_FI - 1) / RS_FI;   // ft_codec_loudness
    int64_t n44[JOIN_MAX_ITEMS], off[JOIN_MAX_ITEMS], raw_off[JOIN_MAX_ITEMS], gaps[JOIN_MAX_ITEMS], raw = 0, need = 0, room = 0;
    int Ls[JOIN_MAX_ITEMS], Ms[JOIN_MAX_ITEMS], Ks[JOIN_MAX_ITEMS];
    bool twin[JOIN_MAX_ITEMS];
    size_t hops = 0;
    for (int b = 0; b < B; ++b) {
        const ft_intake_item& it = items[b];
        const std::string who = fn + ": item " + std::to_string(b);
        if (!it.data || it.n_frames < 1) return ft_fail(ctx, FT_ERR_ARG, who + ": no frames");
        if (it.fmt < IN_U8 || it.fmt > IN_F32) return ft_fail(ctx, FT_ERR_ARG, who + ": fmt outside [0, 4]");
        if (it.channels < 1 || it.channels > 8) return ft_fail(ctx, FT_ERR_ARG, who + ": channels outside [1, 8]");
        if (it.channel < -1 || it.channel >= it.channels) return ft_fail(ctx, FT_ERR_ARG, who + ": channel outside [-1, channels)");
        if (const char* e = chain::rs_design_in(it.rate, &Ls[b], &Ms[b], &Ks[b], nullptr))
            return ft_fail(ctx, FT_ERR_ARG, who + ": " + e + " (" + std::to_string(it.rate) + ")");
        if (it.n_frames > IN_MAX_RAW) return ft_fail(ctx, FT_ERR_TOO_LONG, who + ": more than 2^30 raw bytes in one call");
        const int64_t bytes = it.n_frames * it.channels * IN_WIDTH[it.fmt];
        twin[b] = held && b > 0 && it.data == items[b - 1].data && it.n_frames == items[b - 1].n_frames &&
                  it.channels == items[b - 1].channels && it.fmt == items[b - 1].fmt;     // the other side of a stereo bed:
        raw_off[b] = twin[b] ? raw_off[b - 1] : raw;                                       // its frames are staged once
        if (!twin[b]) raw += (bytes + 15) & ~(int64_t)15;
        if (raw > IN_MAX_RAW) return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": more than 2^30 raw bytes in one call");
        n44[b] = (it.n_frames * Ls[b] + Ms[b] - 1) / Ms[b];
        if (n44[b] > most) return ft_fail(ctx, FT_ERR_TOO_LONG, who + ": longer at 44100 Hz than the longest item the level stage takes");
        hops += level_hops(n44[b], RS_FI);
        room += enc ? (n44[b] + fl - 1) / fl : n44[b];
        gaps[b] = 0;
    }
    if (const char* why = join_check(B, n44, jp, gaps, 0, INT64_MAX, &need)) return ft_fail(ctx, FT_ERR_ARG, fn + ": " + why);
    if (capacity < room) return ft_fail(ctx, FT_ERR_ARG, fn + ": capacity too small");
    const int64_t in_floats = join_offsets(B, n44, off);
    const int R = ctx->cc.n_codebooks + 1;
    std::unique_lock<std::mutex> lock(s->mu, std::defer_lock);
    if (!held) lock.lock();
    FT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = s->stream;
    std::vector<IntakeSeg> segs((size_t)B);
    for (int b = 0; b < B; ++b) {
        const CodecState::RsTab* t = nullptr;
        FT_TRY(in_table(ctx, items[b].rate, &t));
        IntakeSeg& g = segs[b];
        memset(&g, 0, sizeof g);
        g.w = t->K > 0 ? t->w : nullptr;
        g.L = t->L; g.M = t->M; g.K = t->K;
    }
    if (!s->in_seg) {
        FT_TRY(cmalloc(ctx, &s->in_seg, (size_t)JOIN_MAX_ITEMS));
        FT_TRY(cmalloc(ctx, &s->in_count, (size_t)2 * JOIN_MAX_ITEMS));
    }
    FT_TRY(cgrow(ctx, &s->in_raw, &s->in_raw_cap, (size_t)raw));
    if (enc) FT_TRY(cgrow(ctx, &s->in_codes, &s->in_codes_cap, (size_t)room * R));
    FT_TRY(join_alloc(ctx, (size_t)in_floats, (size_t)need));
    FT_TRY(level_alloc(ctx, hops));
    long long mx = 0;
    float* x[JOIN_MAX_ITEMS];
    for (int b = 0; b < B; ++b) {
        const ft_intake_item& it = items[b];
        IntakeSeg& g = segs[b];
        g.raw = s->in_raw + raw_off[b];
        g.y = x[b] = s->join_in + off[b];
        g.count = s->in_count + 2 * b;
        g.n_frames = it.n_frames;
        g.n_out = n44[b];
        g.fmt = it.fmt; g.channels = it.channels; g.channel = it.channel;
        mx = std::max(mx, (long long)n44[b]);
        if (!twin[b])
            FT_HIP(ctx, hipMemcpyAsync(s->in_raw + raw_off[b], it.data, (size_t)(it.n_frames * it.channels * IN_WIDTH[it.fmt]),
                                       hipMemcpyHostToDevice, st));
    }
    FT_HIP(ctx, hipMemsetAsync(s->in_count, 0, (size_t)2 * B * sizeof(unsigned long long), st));
    FT_HIP(ctx, hipMemcpyAsync(s->in_seg, segs.data(), segs.size() * sizeof(IntakeSeg), hipMemcpyHostToDevice, st));
    const int gx = (int)std::max(1LL, std::min(2048LL, (mx + RS_THREADS - 1) / RS_THREADS));
    intake_kernel<<<dim3(gx, 1, (unsigned)B), RS_THREADS, 0, st>>>(s->in_seg);
    unsigned long long count[2 * JOIN_MAX_ITEMS];
    FT_HIP(ctx, hipMemcpyAsync(count, s->in_count, (size_t)2 * B * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    FT_TRY(level_enqueue(ctx, B, x, n44, RS_FI, loudness, loudness != 0));
    int64_t total = 0, cuts[2 * JOIN_MAX_ITEMS];
    FT_TRY(join_run(ctx, B, n44, off, jp, gaps, 0, audio, &total, cuts, need, false, !enc && !held));   // waits for the cuts
    for (int b = 0; b < B; ++b) {
        ft_intake_info& o = infos[b];
        memset(&o, 0, sizeof o);
        o.n44 = n44[b];
        o.a = cuts[2 * b];
        o.e = cuts[2 * b + 1];
        o.clipped = (int64_t)count[2 * b];
        o.nonfinite = (int64_t)count[2 * b + 1];
        const int64_t m = o.e - o.a;
        o.status = m < 1 ? 1 : (fl > 0 && m > (int64_t)s->max_samples) ? 2 : 0;
        o.frames = o.status == 0 && fl > 0 ? (int32_t)((m + fl - 1) / fl) : 0;
        if (lens) lens[b] = m;
    }
    ft_level_info lv[JOIN_MAX_ITEMS];
    level_fetch(s, B, lv);
    for (int b = 0; b < B; ++b) infos[b].level = lv[b];
    if (!enc) return FT_OK;
    // the encoder, clip by clip on the stream; piece b lies at the sum of the pieces before it (no gaps)
    int64_t at = 0, done = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t m = infos[b].e - infos[b].a;
        if (infos[b].status == 0) {
            FT_TRY(encode_enqueue(ctx, s->join_out + at, hipMemcpyDeviceToDevice, m, s->in_codes + done * R, hipMemcpyDeviceToDevice));
            done += infos[b].frames;
        }
        at += m;
    }
    if (done > 0) FT_HIP(ctx, hipMemcpyAsync(codes, s->in_codes, (size_t)done * R * sizeof(int), hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("intake encode launch: ") + hipGetErrorString(e));
    return FT_OK;
}

extern "C" ft_status ft_codec_intake(ft_ctx* ctx, int32_t B, const ft_intake_item* items, const ft_join_params* jp, int32_t loudness,
                                     float* audio, int64_t capacity, int64_t* lens, ft_intake_info* infos) {
    return intake_run(ctx, "ft_codec_intake", B, items, jp, loudness, false, audio, nullptr, capacity, lens, infos);
}

extern "C" ft_status ft_codec_encode_items(ft_ctx* ctx, int32_t B, const ft_intake_item* items, const ft_join_params* jp,
                                           int32_t loudness, int32_t* codes, int64_t capacity_frames, ft_intake_info* infos) {
    return intake_run(ctx, "ft_codec_encode_items", B, items, jp, loudness, true, nullptr, codes, capacity_frames, nullptr, infos);
}

// ---- mix stage (fishtts_hip.h: ft_codec_mix, ft_mix_plan, ft_mix_gains; the kernels in stage_kernels.h, the checks, the hop
// and the table in fx_chain.h).  The four mix stages - mix, stereo mix, live mix, live stereo mix - share one host path:
// mix_args / mix_refuse judge the values, mix_bed prepares the bed, mix_whole is the whole-call walk of the first two,
// ml_begin / ml_push / ml_live the stream of the last two; `pans` (a region table) is what makes a call or a push stereo.
static_assert(sizeof(ft_mix_params) == 72 && offsetof(ft_mix_params, lead) == 24 && offsetof(ft_mix_params, loop) == 64, "ft_mix_params layout");
static_assert(sizeof(ft_mix_info) == 128 && offsetof(ft_mix_info, bed) == 48, "ft_mix_info layout");

extern "C" ft_status ft_mix_gains(float* table) {
    if (!table) return FT_ERR_ARG;
    chain::mx_gains(table);
    return FT_OK;
}

extern "C" ft_status ft_mix_plan(int32_t sample_rate, int64_t n, int64_t lead, int64_t tail, int64_t* N, int32_t* hop, int64_t* nodes) {
    chain::MxArgs a;
    a.rate = sample_rate; a.n = n; a.lead = lead; a.tail = tail;
    bool too_long = false;
    if (chain::mx_check(a, &too_long)) return too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG;
    const chain::MxPlan p = chain::mx_plan(sample_rate, n, lead, tail);
    if (N) *N = p.N;
    if (hop) *hop = p.H;
    if (nodes) *nodes = p.Nh + 1;
    return FT_OK;
}

// T on the device, and the words ft_codec_mix reduces into: uploaded with the first mixed call.
static ft_status mix_table(ft_ctx* ctx) {
    CodecState* s = ctx->codec;
    if (s->mx_T) return FT_OK;
    std::vector<float> T(chain::MX_MAX_DEPTH + 1);
    chain::mx_gains(T.data());
    float* t = nullptr;
    FT_TRY(cmalloc(ctx, &t, T.size()));
    FT_TRY(cupload(ctx, t, T.data(), T.size() * sizeof(float)));
    FT_TRY(cmalloc(ctx, &s->mx_out, (size_t)1));
    s->mx_T = t;
    return FT_OK;
}

// ---- stereo mix stage (fishtts_hip.h: "Stereo mix"; mix_stereo_kernel and the pair level's two kernels in stereo_kernels.h,
// the region checks, the pan table and the side selection in fx_chain.h)
static_assert(sizeof(ft_pan_region) == sizeof(chain::MsRegion) && sizeof(ft_pan_region) == sizeof(MixPan) &&
              offsetof(ft_pan_region, pan) == offsetof(chain::MsRegion, pan) && offsetof(ft_pan_region, pan) == offsetof(MixPan, pan) &&
              offsetof(ft_pan_region, e) == 8 && sizeof(ft_pan_region) == 24, "ft_pan_region layout");
static_assert(2 * chain::MS_MAX_PAN + 1 == MS_PANS && chain::MS_MAX_PAN == MS_CENTRE && MX_SPAN == 4096,
              "fx_chain.h and stereo_kernels.h disagree on the stereo mix stage");

extern "C" ft_status ft_pan_gains(float* table) {
    if (!table) return FT_ERR_ARG;
    chain::ms_gains(table);
    return FT_OK;
}

// U on the device: uploaded with the first stereo call.
static ft_status pan_table(ft_ctx* ctx) {
    CodecState* s = ctx->codec;
    if (s->mx_U) return FT_OK;
    float U[MS_PANS], *u = nullptr;
    chain::ms_gains(U);
    FT_TRY(cmalloc(ctx, &u, (size_t)MS_PANS));
    FT_TRY(cupload(ctx, u, U, sizeof U));
    s->mx_U = u;
    return FT_OK;
}

// The pair level over the two sides of n samples each that intake_run has just left back to back in join_out, their hop sums
// and peaks back to back in the level stage's buffers (s->mu held): the sums added, one gain toward `target`, both sides
// scaled by it.  Waits, and leaves the pair's ft_level_info in *out.
static ft_status level_pair(ft_ctx* ctx, int64_t n, int target, ft_level_info* out) {
    CodecState* s = ctx->codec;
    hipStream_t st = s->stream;
    const long long nh = (long long)level_hops(n, RS_FI);
    s->lv_up.assign(sizeof(LevelTab), 0);
    LevelTab* h = (LevelTab*)s->lv_up.data();
    chain::lv_design(RS_FI, h->c);
    h->ceiling = chain::lv_ceiling();
    h->H = chain::lv_hop(RS_FI);
    h->B = 1;
    h->it[0].x = s->join_out;
    h->it[0].n = n;
    h->it[0].hop0 = 0;
    h->it[0].target = target;
    const size_t used = offsetof(LevelTab, it) + sizeof(LevelItem);
    FT_HIP(ctx, hipMemcpyAsync(s->lv_tab, h, used, hipMemcpyHostToDevice, st));
    level_pair_kernel<<<(unsigned)std::max(1LL, std::min(1024LL, (nh + LV_SCALE_THREADS - 1) / LV_SCALE_THREADS)), LV_SCALE_THREADS, 0, st>>>(
        s->lv_hops, s->lv_peaks, nh);
    level_gain_kernel<<<1, LV_GAIN_THREADS, 0, st>>>(s->lv_tab, s->lv_hops, s->lv_peaks);
    if (target != 0) {
        const int gx = (int)std::max(1LL, std::min(1024LL, (2 * (long long)n + LV_SCALE_THREADS - 1) / LV_SCALE_THREADS));
        level_pair_scale_kernel<<<gx, LV_SCALE_THREADS, 0, st>>>(s->lv_tab);
    }
    s->lv_down.resize(sizeof(LevelTab));
    FT_HIP(ctx, hipMemcpyAsync(s->lv_down.data(), s->lv_tab, used, hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    level_fetch(s, 1, out);
    return FT_OK;
}

// ---- what the four mix stages share on the host: the judged values, the prepared bed, the whole-call walk
static chain::MxArgs mix_args(int rate, int64_t n, const ft_mix_params* mp) {
    chain::MxArgs a;
    a.rate = rate; a.n = n; a.bed_loudness = mp->bed_loudness; a.depth = mp->depth; a.threshold = mp->threshold;
    a.attack = mp->attack; a.release = mp->release; a.lead = mp->lead; a.tail = mp->tail; a.fade_in = mp->fade_in;
    a.fade_out = mp->fade_out; a.offset = mp->offset; a.loop = mp->loop;
    return a;
}
// mx_check's refusal as the entry point `fn` reports it (min_n, pans: as mx_check takes them).
static ft_status mix_refuse(ft_ctx* ctx, const std::string& fn, int rate, int64_t n, const ft_mix_params* mp, long long min_n,
                            const chain::MsTable* pans) {
    bool too_long = false;
    const char* why = chain::mx_check(mix_args(rate, n, mp), &too_long, min_n, pans);
    return why ? ft_fail(ctx, too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG, fn + ": " + why) : FT_OK;
}

template <typename T>
static ft_status ml_malloc(ft_ctx* ctx, ft_mix_stream* ms, T** p, size_t n);   // (an allocation a mix stream owns: below)

// The bed of a mix call or a mix stream (s->mu held; the bed's own checks come before its first device work): raw frames ->
// 44100 Hz by the intake launches, nothing trimmed - one side levelled there; with `stereo`, where the file has two, both
// sides measured as a pair - then each side to the output rate, the whole clip from zero state in one final call
// (resample_kernel; at 44100 Hz its copy mode).  The sides land in an allocation of the stream `ms`, or for a whole call
// (ms null) in the context's mx_bed, side 1 on a 16-byte pitch; a whole call reads one side at 44100 Hz where the intake
// left it, nothing launched.  A null bed (the stereo forms take one): nb = 0, nothing loops, a zeroed report.
// The launch is enqueued, not awaited: g is read by an asynchronous copy and lives until the caller's next wait.
struct MixBed {
    const float* side[2] = {nullptr, nullptr};        // side[1] is side[0] where both sides are one
    int64_t nb = 0, off = 0;                          // samples at the output rate; the bed sample under timeline sample 0
    int loop = 0;
    ft_intake_info info;                              // two sides: clipped and nonfinite summed, the pair's level
    RsSeg g[2];
};
static ft_status mix_bed(ft_ctx* ctx, const std::string& fn, int rate, const ft_intake_item* bed, const ft_mix_params* mp, bool stereo,
                         ft_mix_stream* ms, MixBed* b) {
    CodecState* s = ctx->codec;
    memset(&b->info, 0, sizeof b->info);
    if (!bed) return FT_OK;
    const chain::MsSides sd = stereo ? chain::ms_sides(mp->channel, bed->channels) : chain::MsSides();
    const int sides = sd.same ? 1 : 2;
    ft_intake_item item[2] = {*bed, *bed};
    item[0].channel = sd.same ? mp->channel : sd.ch[0];
    item[1].channel = sd.ch[1];
    const ft_join_params whole = {0.f, 1, 0, 0};
    int64_t lens[2] = {0, 0};
    ft_intake_info bi[2];
    FT_TRY(intake_run(ctx, fn, sides, item, &whole, sd.same ? mp->bed_loudness : 0, false, nullptr, nullptr, INT64_MAX, lens, bi, true));
    const int64_t nb44 = lens[0];
    if (nb44 < 1) return ft_fail(ctx, FT_ERR_ARG, fn + ": the bed has no samples");
    b->info = bi[0];
    if (!sd.same) {
        b->info.clipped += bi[1].clipped;
        b->info.nonfinite += bi[1].nonfinite;
        FT_TRY(level_pair(ctx, nb44, mp->bed_loudness, &b->info.level));
    }
    const CodecState::RsTab* rs = nullptr;
    FT_TRY(rs_table(ctx, rate, &rs));
    const int64_t nb = rs->K > 0 ? (nb44 * rs->L + rs->M - 1) / rs->M : nb44;
    const int64_t pitch = (nb + 3) & ~(int64_t)3;     // side 1 begins on a 16-byte boundary
    b->nb = nb;
    b->off = mp->loop ? mp->offset % nb : std::min(mp->offset, nb);
    b->loop = mp->loop;
    if (!ms && sides == 1 && rs->K == 0) {
        b->side[0] = b->side[1] = s->join_out;
        return FT_OK;
    }
    float* to = nullptr;
    if (ms) {
        FT_TRY(ml_malloc(ctx, ms, &to, (size_t)(pitch * sides)));
    } else {
        FT_TRY(cgrow(ctx, &s->mx_bed, &s->mx_bedcap, (size_t)(pitch * sides)));
        to = s->mx_bed;
    }
    if (!s->rs_seg) FT_TRY(cmalloc(ctx, &s->rs_seg, (size_t)RS_MAX_SEGS));
    for (int c = 0; c < sides; ++c) {
        b->g[c] = RsSeg{s->join_out + c * nb44, rs->K > 0 ? rs->w : nullptr, nullptr, nullptr, to + c * pitch, 0, 0,
                        (int)nb44, (int)nb, rs->L, rs->M, rs->K, 0};
        b->side[c] = to + c * pitch;
    }
    if (sides == 1) b->side[1] = b->side[0];
    FT_HIP(ctx, hipMemcpyAsync(s->rs_seg, b->g, (size_t)sides * sizeof(RsSeg), hipMemcpyHostToDevice, s->stream));
    const int gx = (int)std::max(1LL, std::min(2048LL, ((long long)nb + RS_THREADS - 1) / RS_THREADS));
    resample_kernel<<<dim3(gx, 1, sides), RS_THREADS, 0, s->stream>>>(s->rs_seg);
    return FT_OK;
}

// The mix stage on a whole programme (ft_codec_mix), and with `pans` the stereo mix stage (ft_codec_mix_stereo): two floats
// per frame out, the programme panned by the regions, the bed's sides kept apart, and the bed may be null.  The entry point
// has judged its pointers.  Two waits: the peak decides whether the fourth launch runs.
static ft_status mix_whole(ft_ctx* ctx, const std::string& fn, const float* x, int64_t n, int rate, const chain::MsTable* pans,
                           const ft_intake_item* bed, const ft_mix_params* mp, float* y, int64_t capacity, int64_t* total,
                           int32_t* duck, ft_mix_info* info) {
    FT_TRY(mix_refuse(ctx, fn, rate, n, mp, 1, pans));
    const chain::MxPlan pl = chain::mx_plan(rate, n, mp->lead, mp->tail);
    if (capacity < pl.N) return ft_fail(ctx, FT_ERR_ARG, fn + ": capacity below lead + n + tail");
    CodecState* s = ctx->codec;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, fn, rate, 100, 0, &d));
    const int ch = pans ? 2 : 1, R = pans ? (int)pans->R : 0;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));           // (a call without a bed does not pass through intake_run)
    hipStream_t st = s->stream;
    MixBed b;
    FT_TRY(mix_bed(ctx, fn, rate, bed, mp, pans != nullptr, nullptr, &b));
    FT_TRY(mix_table(ctx));
    if (pans) {
        FT_TRY(pan_table(ctx));
        FT_TRY(cgrow(ctx, &s->mx_reg, &s->mx_regcap, (size_t)std::max(R, 1)));
    }
    FT_TRY(cgrow(ctx, &s->mx_x, &s->mx_xcap, (size_t)n));
    FT_TRY(cgrow(ctx, &s->mx_y, &s->mx_ycap, (size_t)(ch * pl.N)));
    FT_TRY(cgrow(ctx, &s->mx_act, &s->mx_actcap, (size_t)pl.Nh));
    FT_TRY(cgrow(ctx, &s->mx_D, &s->mx_Dcap, (size_t)pl.Nh + 1));
    FT_TRY(cgrow(ctx, &s->mx_g, &s->mx_gcap, (size_t)pl.Nh + 1));
    MixSP sp;                                         // (the mono kernels take its MixP alone)
    memset(&sp, 0, sizeof sp);
    MixP& p = sp.m;
    p.x = s->mx_x; p.bed = b.side[0]; p.T = s->mx_T; p.act = s->mx_act; p.D = s->mx_D; p.g = s->mx_g; p.y = s->mx_y; p.out = s->mx_out;
    p.nb = b.nb; p.off = b.off;
    p.N = (int)pl.N; p.n = (int)n; p.lead = (int)mp->lead; p.Nh = (int)pl.Nh; p.H = pl.H;
    p.depth = mp->depth; p.Wa = mp->attack; p.Wr = mp->release;
    p.f_in = (int)std::min(mp->fade_in, (int64_t)(pl.N / 2)); p.f_out = (int)std::min(mp->fade_out, (int64_t)(pl.N / 2));
    p.loop = b.loop; p.thr = mp->threshold;
    FT_HIP(ctx, hipMemcpyAsync(s->mx_x, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    if (pans) {
        sp.bed1 = b.side[1]; sp.reg = s->mx_reg; sp.U = s->mx_U; sp.R = R;
        if (R > 0) FT_HIP(ctx, hipMemcpyAsync(s->mx_reg, pans->reg, (size_t)R * sizeof(MixPan), hipMemcpyHostToDevice, st));
    }
    FT_HIP(ctx, hipMemsetAsync(s->mx_out, 0, sizeof(MixOut), st));
    mix_hop_kernel<<<(unsigned)((pl.Nh + MX_THREADS / 64 - 1) / (MX_THREADS / 64)), MX_THREADS, 0, st>>>(p);
    mix_node_kernel<<<(unsigned)((pl.Nh + 1 + MX_THREADS - 1) / MX_THREADS), MX_THREADS, 0, st>>>(p);
    if (pans) mix_stereo_kernel<<<(unsigned)((pl.N + MX_SPAN - 1) / MX_SPAN), MX_THREADS, 0, st>>>(sp);
    else mix_kernel<<<(unsigned)((pl.N + MX_SPAN - 1) / MX_SPAN), MX_THREADS, 0, st>>>(p);
    MixOut out;
    FT_HIP(ctx, hipMemcpyAsync(&out, s->mx_out, sizeof out, hipMemcpyDeviceToHost, st));
    if (duck) FT_HIP(ctx, hipMemcpyAsync(duck, s->mx_D, ((size_t)pl.Nh + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));            // the peak decides whether the fourth launch runs
    float pk, sg = 1.f;
    memcpy(&pk, &out.pk, sizeof pk);
    const bool capped = (double)pk > chain::lv_ceiling();
    if (capped) {
        sg = (float)(chain::lv_ceiling() / (double)pk);
        const int gx = (int)std::max(1LL, std::min(4096LL, (ch * pl.N / 4 + MX_THREADS - 1) / MX_THREADS));
        mix_scale_kernel<<<gx, MX_THREADS, 0, st>>>(s->mx_y, (int)(ch * pl.N), sg);
    }
    FT_HIP(ctx, hipMemcpyAsync(y, s->mx_y, (size_t)(ch * pl.N) * sizeof(float), hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, fn + " launch: " + hipGetErrorString(e));
    *total = pl.N;
    memset(info, 0, sizeof *info);
    info->N = pl.N; info->nb = b.nb; info->Nh = pl.Nh; info->active = out.active;
    info->dmax = out.dmax; info->capped = capped ? 1 : 0; info->pk = pk; info->sg = sg;
    info->bed = b.info;
    return FT_OK;
}

extern "C" ft_status ft_codec_mix(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_intake_item* bed,
                                  const ft_mix_params* mp, float* y, int64_t capacity, int64_t* total, int32_t* duck, ft_mix_info* info) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!x || !bed || !mp || !y || !total || !info) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_mix: a null pointer");
    return mix_whole(ctx, "ft_codec_mix", x, n, sample_rate, nullptr, bed, mp, y, capacity, total, duck, info);
}

extern "C" ft_status ft_codec_mix_stereo(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_pan_region* regions,
                                         int32_t R, const ft_intake_item* bed, const ft_mix_params* mp, float* y, int64_t capacity,
                                         int64_t* total, int32_t* duck, ft_mix_info* info) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!x || !mp || !y || !total || !info) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_mix_stereo: a null pointer");
    const chain::MsTable pans = {(const chain::MsRegion*)regions, R};
    return mix_whole(ctx, "ft_codec_mix_stereo", x, n, sample_rate, &pans, bed, mp, y, capacity, total, duck, info);
}

// ---- room stage (fishtts_hip.h: "Room"; the kernels in room_kernels.h, the checks, L, f, N and the sizes in fx_chain.h).
// The impulse response comes through mix_bed - the intake launches and the resampler as Mix prepares its bed.
static_assert(sizeof(ft_send_region) == sizeof(chain::MsRegion) && offsetof(ft_send_region, send) == offsetof(MixPan, pan) &&
              sizeof(ft_send_region) == sizeof(MixPan), "ft_send_region layout");
static_assert(sizeof(ft_room_params) == 64 && offsetof(ft_room_params, offset) == 24, "ft_room_params layout");
static_assert(sizeof(ft_room_info) == 128 && offsetof(ft_room_info, ir) == 48, "ft_room_info layout");
static_assert(chain::RM_MAX_L == RM_MAX_L && RM_BLOCK == 256 && RM_DC % RM_STEP == 0 && RM_STEP % 2 == 0 && RM_LAUNCH % RM_SPAN == 0,
              "fx_chain.h and room_kernels.h disagree on the room stage");

static chain::RmArgs room_args(int rate, int64_t n, const ft_intake_item* ir, const ft_room_params* rp) {
    chain::RmArgs a;
    a.rate = rate; a.n = n; a.channel = rp->channel; a.normalize = rp->normalize; a.wet = rp->wet; a.dry = rp->dry;
    a.send = rp->send; a.ceiling = rp->ceiling; a.offset = rp->offset; a.length = rp->length; a.fade = rp->fade;
    a.predelay = rp->predelay; a.tail = rp->tail;
    a.ir_rate = ir->rate; a.ir_channels = ir->channels; a.ir_frames = ir->n_frames;
    return a;
}

extern "C" ft_status ft_room_plan(int32_t sample_rate, int64_t n, int64_t nh, const ft_room_params* rp, int64_t* L, int64_t* N) {
    if (!rp || nh < 0) return FT_ERR_ARG;
    const ft_intake_item it = {nullptr, 1, chain::RS_FI, rp->channel < 0 ? 1 : rp->channel + 1, 0, 0};   // (no item: its checks pass)
    chain::RmArgs a = room_args(sample_rate, n, &it, rp);
    a.nh = nh;
    bool too_long = false;
    chain::RmPlan pl;
    if (chain::rm_check(a, chain::MsTable(), &too_long, &pl)) return too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG;
    if (L) *L = pl.L;
    if (N) *N = pl.N;
    return FT_OK;
}

// The chain's launches over outputs [0, N) (s->mu held): RM_LAUNCH outputs each.
static void room_conv(CodecState* s, RoomConvP p) {
    for (long long i0 = 0; i0 < p.N; i0 += RM_LAUNCH) {
        p.i0 = (int)i0;
        const long long span = std::min<long long>(RM_LAUNCH, p.N - i0);
        room_conv_kernel<<<(unsigned)((span + RM_SPAN - 1) / RM_SPAN), RM_THREADS, 0, s->stream>>>(p);
    }
}

static ft_status room_out(ft_ctx* ctx) {
    CodecState* s = ctx->codec;
    if (!s->rm_out) FT_TRY(cmalloc(ctx, &s->rm_out, (size_t)1));
    return FT_OK;
}

extern "C" ft_status ft_codec_room(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_send_region* regions,
                                   int32_t R, const ft_intake_item* ir, const ft_room_params* rp, float* y, int64_t capacity,
                                   int64_t* total, ft_room_info* info) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    const std::string fn = "ft_codec_room";
    if (!x || !ir || !rp || !y || !total || !info) return ft_fail(ctx, FT_ERR_ARG, fn + ": a null pointer");
    const chain::MsTable regs = {(const chain::MsRegion*)regions, R};
    const chain::RmArgs a = room_args(sample_rate, n, ir, rp);
    bool too_long = false;
    chain::RmPlan pl;
    if (const char* why = chain::rm_check(a, regs, &too_long, &pl))
        return ft_fail(ctx, too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG, fn + ": " + why);
    if (pl.nh >= 0 && capacity < pl.N) return ft_fail(ctx, FT_ERR_ARG, fn + ": capacity below n + tail");
    CodecState* s = ctx->codec;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, fn, sample_rate, 100, 0, &d));
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = s->stream;
    ft_mix_params mp;
    memset(&mp, 0, sizeof mp);
    mp.channel = rp->channel;
    MixBed b;
    FT_TRY(mix_bed(ctx, fn, sample_rate, ir, &mp, false, nullptr, &b));
    if (b.nb != pl.nh) return ft_fail(ctx, FT_ERR_STATE, fn + ": the impulse response's length is not the planned one");
    FT_TRY(mix_table(ctx));
    FT_TRY(room_out(ctx));
    const chain::RmSizes z = chain::rm_sizes(a, pl);
    FT_TRY(cgrow(ctx, &s->mx_x, &s->mx_xcap, z.x));
    FT_TRY(cgrow(ctx, &s->mx_y, &s->mx_ycap, z.y));
    FT_TRY(cgrow(ctx, &s->rm_t, &s->rm_tcap, z.taps));
    FT_TRY(cgrow(ctx, &s->rm_hn, &s->rm_hncap, z.taps));
    FT_TRY(cgrow(ctx, &s->rm_e, &s->rm_ecap, z.blocks));
    if (pl.send) {
        FT_TRY(cgrow(ctx, &s->rm_xs, &s->rm_xscap, z.xs));
        FT_TRY(cgrow(ctx, &s->mx_reg, &s->mx_regcap, (size_t)std::max(R, 1)));
    }
    std::vector<float> T(chain::MX_MAX_DEPTH + 1);
    chain::mx_gains(T.data());
    FT_HIP(ctx, hipMemcpyAsync(s->mx_x, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    FT_HIP(ctx, hipMemsetAsync(s->rm_out, 0, sizeof(RoomOut), st));
    RoomIrP ip = {b.side[0], s->rm_t, s->rm_hn, s->rm_e, s->rm_out, (int)pl.L, (int)pl.f, rp->normalize, rp->offset};
    room_ir_kernel<<<(unsigned)((z.blocks + 63) / 64), 64, 0, st>>>(ip);
    room_gain_kernel<<<1, 1024, 0, st>>>(ip);
    if (pl.send) {
        if (R > 0) FT_HIP(ctx, hipMemcpyAsync(s->mx_reg, regions, (size_t)R * sizeof(MixPan), hipMemcpyHostToDevice, st));
        RoomSendP sp = {s->mx_x, s->rm_xs, s->mx_T, s->mx_reg, (int)n, R, rp->send};
        room_send_kernel<<<(unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)), 256, 0, st>>>(sp);
    }
    RoomConvP cp;
    memset(&cp, 0, sizeof cp);
    cp.xs = pl.send ? s->rm_xs : s->mx_x; cp.x = s->mx_x; cp.hn = s->rm_hn; cp.y = s->mx_y; cp.out = s->rm_out;
    cp.n = (int)n; cp.L = (int)pl.L; cp.predelay = (int)rp->predelay; cp.N = (int)pl.N;
    cp.dry = rp->dry >= 0; cp.gd = cp.dry ? T[rp->dry] : 0.f; cp.gw = T[rp->wet];
    room_conv(s, cp);
    RoomOut out;
    FT_HIP(ctx, hipMemcpyAsync(&out, s->rm_out, sizeof out, hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));            // E may refuse the call; the peak decides whether the last launch runs
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, fn + " launch: " + hipGetErrorString(e));
    if (rp->normalize && (!(out.E > 0.0) || !std::isfinite(out.E)))
        return ft_fail(ctx, FT_ERR_ARG, fn + ": the impulse response's energy is zero or not finite");
    float pk, sg = 1.f;
    memcpy(&pk, &out.pk, sizeof pk);
    const bool capped = rp->ceiling && (double)pk > chain::lv_ceiling();
    if (capped) {
        sg = (float)(chain::lv_ceiling() / (double)pk);
        const int gx = (int)std::max(1LL, std::min(4096LL, (pl.N / 4 + MX_THREADS - 1) / MX_THREADS));
        mix_scale_kernel<<<gx, MX_THREADS, 0, st>>>(s->mx_y, (int)pl.N, sg);
    }
    FT_HIP(ctx, hipMemcpyAsync(y, s->mx_y, (size_t)pl.N * sizeof(float), hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, fn + " launch: " + hipGetErrorString(e));
    *total = pl.N;
    memset(info, 0, sizeof *info);
    info->N = pl.N; info->nh = pl.nh; info->L = pl.L; info->E = out.E; info->gn = out.gn; info->pk = pk; info->sg = sg;
    info->capped = capped ? 1 : 0;
    info->ir = b.info;
    return FT_OK;
}

// ---- FLAC stage (flac_kernels.h; fishtts_hip.h states it, flac_plan.h checks and sizes it)
static_assert(sizeof(ft_flac_info) == 72 && offsetof(ft_flac_info, kinds) == 24 && sizeof(ft_flac_params) == 8, "ft_flac_info layout");
static_assert(sizeof(FlSig) == 8 + FL_FINE && FL_THREADS == FL_FINE, "a thread per finest partition");

extern "C" int64_t ft_flac_bound(int64_t n, int32_t channels, int32_t blocksize) { return flac::fl_bound(n, channels, blocksize); }

// The four frame launches over n frames of samples that lie on the device (s->mu held): the buffers grown for F frames and
// `bound` stream bytes (the 42 counted), the counters zeroed, the frames numbered from f0, FlacOut read back and judged.
static ft_status flac_frames(ft_ctx* ctx, const std::string& fn, const void* dx, int fmt, long long n, int channels, int B, int rate,
                             long long f0, long long bound, FlacOut* o) {
    CodecState* s = ctx->codec;
    hipStream_t st = s->stream;
    const long long F = flac::fl_frames(n, B);
    const int nsig = channels == 2 ? 4 : 1;
    const size_t stride = (size_t)((flac::fl_frame_bound(B, channels) + 3) / 4 * 4);
    FT_TRY(cgrow(ctx, &s->fl_sig, &s->fl_sigcap, (size_t)F * nsig));
    FT_TRY(cgrow(ctx, &s->fl_slots, &s->fl_slotcap, (size_t)F * stride + 8));
    FT_TRY(cgrow(ctx, &s->fl_len, &s->fl_lencap, (size_t)F));
    FT_TRY(cgrow(ctx, &s->fl_off, &s->fl_offcap, (size_t)F));
    FT_TRY(cgrow(ctx, &s->fl_stream, &s->fl_streamcap, (size_t)bound + 8));
    if (!s->fl_out) FT_TRY(cmalloc(ctx, &s->fl_out, (size_t)1));
    FT_HIP(ctx, hipMemsetAsync(s->fl_out, 0, sizeof(FlacOut), st));
    FlacP p;
    memset(&p, 0, sizeof p);
    p.x = dx; p.n = n; p.fmt = fmt; p.channels = channels; p.B = B; p.rate = rate; p.F = (int)F; p.nsig = nsig;
    p.sig = s->fl_sig; p.slots = s->fl_slots; p.stride = (int)stride; p.flen = s->fl_len; p.foff = s->fl_off;
    p.stream = s->fl_stream; p.out = s->fl_out; p.f0 = f0;
    flac_analyse_kernel<<<dim3((unsigned)F, (unsigned)nsig), FL_THREADS, 0, st>>>(p);
    flac_pack_kernel<<<(unsigned)F, FL_THREADS, 0, st>>>(p);
    flac_scan_kernel<<<1, FL_SCAN_THREADS, 0, st>>>(p);
    flac_gather_kernel<<<(unsigned)F, FL_THREADS, 0, st>>>(p);
    FT_HIP(ctx, hipMemcpyAsync(o, s->fl_out, sizeof *o, hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));              // the stream's length decides how much comes back
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, fn + " launch: " + hipGetErrorString(e));
    if (o->overflow != 0) return ft_fail(ctx, FT_ERR_STATE, fn + ": a frame did not fit its bound");
    if (o->total < flac::FL_STREAM_HEAD || o->total > bound || o->frames != (int)F)
        return ft_fail(ctx, FT_ERR_STATE, fn + ": the stream's length is not within the bound");
    return FT_OK;
}

extern "C" ft_status ft_codec_flac(ft_ctx* ctx, const void* x, int32_t fmt, int64_t n, int32_t channels, int32_t sample_rate,
                                   const ft_flac_params* fp, uint8_t* out, int64_t capacity, int64_t* total, ft_flac_info* info) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    const std::string fn = "ft_codec_flac";
    if (!x || !fp || !out || !total || !info) return ft_fail(ctx, FT_ERR_ARG, fn + ": a null pointer");
    flac::FlArgs a;
    a.fmt = fmt; a.channels = channels; a.rate = sample_rate; a.blocksize = fp->blocksize; a.reserved = fp->reserved;
    a.n = n; a.capacity = capacity;
    bool too_long = false;
    if (const char* why = flac::fl_check(a, &too_long)) return ft_fail(ctx, too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG, fn + ": " + why);
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = s->stream;
    const int B = fp->blocksize;
    const size_t in_bytes = (size_t)n * channels * (fmt ? 2 : 4);
    FT_TRY(cgrow(ctx, &s->fl_in, &s->fl_incap, in_bytes));
    FT_HIP(ctx, hipMemcpyAsync(s->fl_in, x, in_bytes, hipMemcpyHostToDevice, st));
    FlacOut o;
    FT_TRY(flac_frames(ctx, fn, s->fl_in, fmt, n, channels, B, sample_rate, 0, flac::fl_bound(n, channels, B), &o));
    FT_HIP(ctx, hipMemcpyAsync(out, s->fl_stream, (size_t)o.total, hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    *total = o.total;
    memset(info, 0, sizeof *info);
    info->frames = o.frames; info->bytes = o.total; info->min_frame = o.fmin; info->max_frame = o.fmax;
    for (int i = 0; i < flac::FL_KINDS; ++i) info->kinds[i] = o.kinds[i];
    for (int i = 0; i < flac::FL_ASSIGNMENTS; ++i) info->assignments[i] = o.assignments[i];
    return FT_OK;
}

// ---- live FLAC stage (fishtts_hip.h: "Live FLAC"; flacl_stage_kernel in flac_kernels.h; the emission rule, the host state and
// the per-push checks in flac_plan.h).  A stream owns two copies of its carry, allocated at `begin`; a push stages its raw
// samples in fl_in and carry || push in fl_stage, runs the FLAC stage's launches on that and ends with a wait, so nothing of a
// push outlives it, and the host state moves only when the launches went through.
struct ft_flac_stream {
    ft_ctx* owner = nullptr;          // null once its context is gone (the device state went with it)
    flac::FlStream st;
    short* carry[2] = {nullptr, nullptr};
};

static void flac_stream_orphan(ft_flac_stream* fs) {
    for (int c = 0; c < 2; ++c) {
        if (fs->carry[c]) hipFree(fs->carry[c]);
        fs->carry[c] = nullptr;
    }
    fs->owner = nullptr;
}

static void fls_end(ft_ctx* ctx, ft_flac_stream* fs) {   // (s->mu held)
    CodecState* s = ctx->codec;
    hipStreamSynchronize(s->stream);
    flac_stream_orphan(fs);
    for (size_t i = 0; i < s->flac_streams.size(); ++i)
        if (s->flac_streams[i] == fs) { s->flac_streams.erase(s->flac_streams.begin() + (long)i); break; }
    delete fs;
}

extern "C" ft_status ft_flac_stream_plan(int32_t blocksize, int32_t channels, int64_t before, int64_t n, int32_t final,
                                         int64_t* frames, int64_t* bytes) {
    const int why = flac::fl_push_refused(blocksize, channels, before, n);
    if (why) return why == 2 ? FT_ERR_TOO_LONG : FT_ERR_ARG;
    const flac::FlPush pl = flac::fl_push_plan(blocksize, channels, before, n, final != 0);
    if (frames) *frames = pl.F;
    if (bytes) *bytes = pl.bytes;
    return FT_OK;
}

extern "C" ft_status ft_codec_flac_stream_begin(ft_ctx* ctx, int32_t channels, int32_t fmt, int32_t sample_rate,
                                                const ft_flac_params* fp, ft_flac_stream** out) {
    const std::string fn = "ft_codec_flac_stream_begin";
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!fp || !out) return ft_fail(ctx, FT_ERR_ARG, fn + ": a null pointer");
    if (const char* why = flac::fl_stream_begin_check(fmt, channels, sample_rate, fp->blocksize, fp->reserved))
        return ft_fail(ctx, FT_ERR_ARG, fn + ": " + why);
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    ft_flac_stream* fs = new ft_flac_stream();
    fs->owner = ctx;
    fs->st.fmt = fmt; fs->st.channels = channels; fs->st.rate = sample_rate; fs->st.B = fp->blocksize;
    s->flac_streams.push_back(fs);
    for (int c = 0; c < 2; ++c) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, (size_t)fp->blocksize * channels * sizeof(short) + 64);
        if (e != hipSuccess) {
            fls_end(ctx, fs);
            return ft_fail(ctx, FT_ERR_NOMEM, fn + " hipMalloc: " + hipGetErrorString(e));
        }
        fs->carry[c] = (short*)q;
    }
    *out = fs;
    return FT_OK;
}

extern "C" ft_status ft_codec_flac_stream_push(ft_flac_stream* fs, const void* x, int64_t n, int32_t final, uint8_t* out,
                                               int64_t capacity, int64_t* n_bytes) {
    const std::string fn = "ft_codec_flac_stream_push";
    if (!fs) return FT_ERR_ARG;
    ft_ctx* ctx = fs->owner;
    if (!ctx || !ctx->codec) return FT_ERR_STATE;      // its context was destroyed
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    flac::FlStream& stg = fs->st;
    bool state = false, too_long = false;
    if (const char* why = flac::fl_stream_check(&stg, !out || !n_bytes, !x, n, final != 0, capacity, &state, &too_long))
        return ft_fail(ctx, state ? FT_ERR_STATE : too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG, fn + ": " + why);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = s->stream;
    const flac::FlPush pl = stg.plan(n, final != 0);
    const int ch = stg.channels;
    if (pl.T > 0) {
        const size_t in_bytes = (size_t)n * ch * (stg.fmt ? 2 : 4);
        FT_TRY(cgrow(ctx, &s->fl_in, &s->fl_incap, std::max(in_bytes, (size_t)8)));
        FT_TRY(cgrow(ctx, &s->fl_stage, &s->fl_stagecap, (size_t)pl.T * ch + 4));
        if (n > 0) FT_HIP(ctx, hipMemcpyAsync(s->fl_in, x, in_bytes, hipMemcpyHostToDevice, st));
        FlacStageP q;
        memset(&q, 0, sizeof q);
        q.carry_in = fs->carry[stg.par]; q.carry_out = fs->carry[stg.par ^ 1]; q.stage = s->fl_stage;
        q.push.x = s->fl_in; q.push.fmt = stg.fmt; q.push.channels = ch;
        q.r = pl.r; q.T = pl.T; q.taken = pl.taken;
        const long long groups = (pl.T * ch + 3) / 4;
        flacl_stage_kernel<<<(unsigned)std::max(1LL, std::min(4096LL, (groups + FL_THREADS - 1) / FL_THREADS)), FL_THREADS, 0, st>>>(q);
    }
    FlacOut o;
    memset(&o, 0, sizeof o);
    long long got = 0;
    if (pl.F > 0) {
        FT_TRY(flac_frames(ctx, fn, s->fl_stage, 1, pl.taken, ch, stg.B, stg.rate, stg.F_done, flac::FL_STREAM_HEAD + pl.bytes, &o));
        got = o.total - flac::FL_STREAM_HEAD;
        if (got > 0) FT_HIP(ctx, hipMemcpyAsync(out, s->fl_stream + flac::FL_STREAM_HEAD, (size_t)got, hipMemcpyDeviceToHost, st));
    }
    FT_HIP(ctx, hipStreamSynchronize(st));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, fn + " launch: " + hipGetErrorString(e));
    stg.commit(pl, n, final != 0, got, o.fmin, o.fmax, o.kinds, o.assignments);
    *n_bytes = got;
    return FT_OK;
}

extern "C" ft_status ft_codec_flac_stream_head(ft_flac_stream* fs, uint8_t out[42]) {
    if (!fs || !out) return FT_ERR_ARG;
    ft_ctx* ctx = fs->owner;
    std::unique_lock<std::mutex> lock;
    if (ctx && ctx->codec) lock = std::unique_lock<std::mutex>(ctx->codec->mu);
    fs->st.head(out);
    return FT_OK;
}

extern "C" ft_status ft_codec_flac_stream_info(ft_flac_stream* fs, ft_flac_info* info) {
    if (!fs || !info) return FT_ERR_ARG;
    ft_ctx* ctx = fs->owner;
    std::unique_lock<std::mutex> lock;
    if (ctx && ctx->codec) lock = std::unique_lock<std::mutex>(ctx->codec->mu);
    const flac::FlStream& stg = fs->st;
    memset(info, 0, sizeof *info);
    info->frames = stg.F_done; info->bytes = flac::FL_STREAM_HEAD + stg.bytes; info->min_frame = stg.fmin; info->max_frame = stg.fmax;
    for (int i = 0; i < flac::FL_KINDS; ++i) info->kinds[i] = stg.kinds[i];
    for (int i = 0; i < flac::FL_ASSIGNMENTS; ++i) info->assignments[i] = stg.assignments[i];
    return FT_OK;
}

extern "C" void ft_codec_flac_stream_end(ft_flac_stream* fs) {
    if (!fs) return;
    ft_ctx* own = fs->owner;
    if (own && own->codec) {
        std::lock_guard<std::mutex> lock(own->codec->mu);
        hipSetDevice(own->device);
        fls_end(own, fs);
        return;
    }
    delete fs;
}

extern "C" ft_status ft_test_room_conv(ft_ctx* ctx, const float* xs, int64_t n, const float* hn, int64_t L, int64_t predelay,
                                       int64_t N, float* c) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!xs || !hn || !c || n < 1 || n > chain::MX_MAX_N || L < 1 || L > RM_MAX_L || predelay < 0 || predelay > RS_MAX_RATE || N < 1 ||
        N > chain::MX_MAX_N)
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_room_conv: bad argument");
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = s->stream;
    FT_TRY(room_out(ctx));
    FT_TRY(cgrow(ctx, &s->mx_x, &s->mx_xcap, (size_t)n));
    FT_TRY(cgrow(ctx, &s->mx_y, &s->mx_ycap, (size_t)N));
    FT_TRY(cgrow(ctx, &s->rm_hn, &s->rm_hncap, (size_t)L));
    FT_HIP(ctx, hipMemcpyAsync(s->mx_x, xs, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    FT_HIP(ctx, hipMemcpyAsync(s->rm_hn, hn, (size_t)L * sizeof(float), hipMemcpyHostToDevice, st));
    FT_HIP(ctx, hipMemsetAsync(s->rm_out, 0, sizeof(RoomOut), st));
    RoomConvP cp;
    memset(&cp, 0, sizeof cp);
    cp.xs = cp.x = s->mx_x; cp.hn = s->rm_hn; cp.y = s->mx_y; cp.out = s->rm_out;
    cp.n = (int)n; cp.L = (int)L; cp.predelay = (int)predelay; cp.N = (int)N; cp.raw = 1;
    room_conv(s, cp);
    FT_HIP(ctx, hipMemcpyAsync(c, s->mx_y, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, std::string("ft_test_room_conv launch: ") + hipGetErrorString(e));
    return FT_OK;
}

// ---- live mix stages (fishtts_hip.h: "Live mix", "Live stereo mix"; the kernels in stage_kernels.h and, mixls_*_kernel, in
// stereo_kernels.h; the emission, the stream's counters, the per-push region check, the pan words and the buffer sizes in
// fx_chain.h).  A stream owns its prepared bed, its two pairs of carries, its per-hop arrays and the four words it reports;
// a push stages its samples in the context's buffers and ends with one wait, so nothing of a push outlives it.  A stereo
// stream is a mix stream with two sides of the bed, a pan byte carry beside its programme carry and two floats per frame in
// its m carries and in what it emits.
static_assert(chain::MLS_WORD == 16 && MS_CENTRE == chain::MS_MAX_PAN, "fx_chain.h and stereo_kernels.h disagree on the pan bytes");
static_assert(chain::ML_LA == ML_ATTACK && chain::ML_LR == ML_RELEASE && RS_MAX_RATE / 50 / 4 + 1 <= MX_THREADS &&
              chain::ML_MAX_FADE == (1LL << 30), "fx_chain.h and stage_kernels.h disagree on the live mix stage");
static_assert(sizeof(ft_mix_live_info) == 128 && offsetof(ft_mix_live_info, bed) == 48, "ft_mix_live_info layout");

struct ft_mix_stream {
    ft_ctx* owner = nullptr;          // null once its context is gone (the device state went with it)
    chain::MlStage st;
    ft_mix_params mp;
    int rate = RS_FI;
    bool stereo = false;              // a stream of the live stereo mix stage: two floats per frame in mc and in what it emits
    const float* bed = nullptr;       // the prepared bed at the output rate, nb samples (stereo: side 0, null without a bed)
    const float* bed1 = nullptr;      // side 1, `bed` itself where both sides are one
    unsigned char* pq[2] = {nullptr, nullptr};   // stereo: the pan bytes of the carried programme, laid out as prog
    size_t qcap[2] = {0, 0};
    long long nb = 0, off = 0;
    ft_intake_info binfo;
    float *prog[2] = {nullptr, nullptr}, *mc[2] = {nullptr, nullptr};   // the carries: programme, m
    size_t pcap[2] = {0, 0}, mcap[2] = {0, 0};
    unsigned char* act = nullptr;     // per hop, whole: they grow on need
    int *D = nullptr, *need = nullptr, *L = nullptr;
    float* g = nullptr;
    size_t hcap = 0;
    MixLiveOut* out = nullptr;
    std::vector<void*> owned;
};

static void mix_stream_orphan(ft_mix_stream* ms) {
    for (void* v : ms->owned) hipFree(v);
    ms->owned.clear();
    ms->owner = nullptr;
}

template <typename T>
static ft_status ml_malloc(ft_ctx* ctx, ft_mix_stream* ms, T** p, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (n + 8) * sizeof(T));
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_NOMEM, std::string("mix stream hipMalloc: ") + hipGetErrorString(e));
    ms->owned.push_back(q);
    *p = (T*)q;
    return FT_OK;
}
static void ml_free(ft_mix_stream* ms, void* p) {
    if (!p) return;
    ms->owned.erase(std::find(ms->owned.begin(), ms->owned.end(), p));
    hipFree(p);
}
// A carry copy the next push writes from its first sample on: nothing of it is kept when it has to be larger.
template <typename T>
static ft_status ml_carry(ft_ctx* ctx, ft_mix_stream* ms, T** p, size_t* cap, size_t need) {
    if (*p && *cap >= need) return FT_OK;
    T* q = nullptr;
    FT_TRY(ml_malloc(ctx, ms, &q, need));
    ml_free(ms, *p);
    *p = q;
    *cap = need;
    return FT_OK;
}
// The per-hop arrays with room for `hops` hops and hops + 1 nodes; what they hold moves along.
static ft_status ml_hops(ft_ctx* ctx, ft_mix_stream* ms, size_t hops) {
    if (ms->act && ms->hcap >= hops) return FT_OK;
    const size_t cap = std::max(hops, std::max((size_t)4096, 2 * ms->hcap)), n = cap + 1;
    hipStream_t st = ctx->codec->stream;
    unsigned char* act = nullptr;
    int *D = nullptr, *need = nullptr, *L = nullptr;
    float* g = nullptr;
    FT_TRY(ml_malloc(ctx, ms, &act, n));
    FT_TRY(ml_malloc(ctx, ms, &D, n));
    FT_TRY(ml_malloc(ctx, ms, &g, n));
    FT_TRY(ml_malloc(ctx, ms, &need, n));
    FT_TRY(ml_malloc(ctx, ms, &L, n));
    if (ms->act) {
        const size_t o = ms->hcap + 1;
        FT_HIP(ctx, hipMemcpyAsync(act, ms->act, o, hipMemcpyDeviceToDevice, st));
        FT_HIP(ctx, hipMemcpyAsync(D, ms->D, o * sizeof(int), hipMemcpyDeviceToDevice, st));
        FT_HIP(ctx, hipMemcpyAsync(g, ms->g, o * sizeof(float), hipMemcpyDeviceToDevice, st));
        FT_HIP(ctx, hipMemcpyAsync(need, ms->need, o * sizeof(int), hipMemcpyDeviceToDevice, st));
        FT_HIP(ctx, hipMemcpyAsync(L, ms->L, o * sizeof(int), hipMemcpyDeviceToDevice, st));
        FT_HIP(ctx, hipStreamSynchronize(st));
        ml_free(ms, ms->act); ml_free(ms, ms->D); ml_free(ms, ms->g); ml_free(ms, ms->need); ml_free(ms, ms->L);
    }
    ms->act = act; ms->D = D; ms->g = g; ms->need = need; ms->L = L;
    ms->hcap = cap;
    return FT_OK;
}

static chain::MlShape ml_shape(int rate, const ft_mix_params* mp) {
    chain::MlShape sh;
    sh.H = chain::mx_hop(rate); sh.Wa = mp->attack; sh.lead = mp->lead; sh.tail = mp->tail; sh.fade_out = mp->fade_out;
    return sh;
}

extern "C" ft_status ft_mix_live_plan(int32_t sample_rate, const ft_mix_params* mp, int64_t n_in, int32_t final, int64_t* n_out,
                                      int64_t* nodes) {
    if (!mp) return FT_ERR_ARG;
    bool too_long = false;
    if (chain::mx_check(mix_args(sample_rate, n_in, mp), &too_long, 0)) return too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG;
    const chain::MlPlan p = chain::ml_plan(ml_shape(sample_rate, mp), n_in, final != 0);
    if (n_out) *n_out = p.done;
    if (nodes) *nodes = p.limits;
    return FT_OK;
}

static void ml_end(ft_ctx* ctx, ft_mix_stream* ms) {   // (s->mu held)
    CodecState* s = ctx->codec;
    hipStreamSynchronize(s->stream);
    for (void* v : ms->owned) hipFree(v);
    ms->owned.clear();
    for (size_t i = 0; i < s->mix_streams.size(); ++i)
        if (s->mix_streams[i] == ms) { s->mix_streams.erase(s->mix_streams.begin() + (long)i); break; }
    delete ms;
}

// The stream of a call whose values mx_check has passed (s->mu held): the bed prepared into an allocation of the stream's
// own, the state allocated.  `stereo`: a stream of the live stereo mix stage, whose bed may be null.  A begin that fails
// once the stream exists frees it.
static ft_status ml_begin(ft_ctx* ctx, const std::string& fn, int rate, const ft_intake_item* bed, const ft_mix_params* mp, bool stereo,
                          ft_mix_stream** out) {
    CodecState* s = ctx->codec;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, fn, rate, 100, 0, &d));
    FT_HIP(ctx, hipSetDevice(ctx->device));           // (a stream without a bed does not pass through intake_run)
    hipStream_t st = s->stream;
    ft_mix_stream* ms = new ft_mix_stream();
    ms->owner = ctx;
    ms->stereo = stereo;
    ms->mp = *mp;
    ms->rate = rate;
    ms->st = chain::MlStage::fresh(ml_shape(rate, mp));
    s->mix_streams.push_back(ms);
    MixBed b;                                         // (alive until the wait below)
    ft_status r = mix_bed(ctx, fn, rate, bed, mp, stereo, ms, &b);
    if (r == FT_OK) r = mix_table(ctx);
    if (r == FT_OK && stereo) r = pan_table(ctx);
    if (r == FT_OK) r = ml_malloc(ctx, ms, &ms->out, (size_t)1);
    if (r == FT_OK) r = ml_hops(ctx, ms, 1);
    for (int c = 0; c < 2 && r == FT_OK; ++c) {
        r = ml_carry(ctx, ms, &ms->prog[c], &ms->pcap[c], 4);
        if (r == FT_OK && stereo) r = ml_carry(ctx, ms, &ms->pq[c], &ms->qcap[c], 4);
        if (r == FT_OK) r = ml_carry(ctx, ms, &ms->mc[c], &ms->mcap[c], stereo ? 8 : 4);
    }
    if (r == FT_OK) {
        hipError_t e = hipMemsetAsync(ms->out, 0, sizeof(MixLiveOut), st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) r = ft_fail(ctx, FT_ERR_HIP, fn + ": " + hipGetErrorString(e));
    }
    if (r != FT_OK) {
        ml_end(ctx, ms);
        return r;
    }
    ms->bed = b.side[0];
    ms->bed1 = b.side[1];
    ms->nb = b.nb;
    ms->off = b.off;
    ms->mp.loop = b.loop;                             // (without a bed nothing loops: nb = 0)
    ms->binfo = b.info;
    *out = ms;
    return FT_OK;
}

// The launch parameters of a push with plan pl (the staged buffers are the context's).
static MixLiveP ml_fill(CodecState* s, const ft_mix_stream* ms, const chain::MlPlan& pl, bool final) {
    const chain::MlStage& stg = ms->st;
    const int H = stg.s.H, w = stg.par ^ 1;
    const long long F0 = stg.s.lead + stg.nin, mend0 = stg.mixed * H, mend1 = final ? pl.N : pl.mixed * H;
    MixLiveP p;
    memset(&p, 0, sizeof p);
    p.m.x = s->ml_x; p.m.bed = ms->bed; p.m.T = s->mx_T; p.m.act = ms->act; p.m.D = ms->D; p.m.g = ms->g; p.m.y = s->ml_m;
    p.m.nb = ms->nb; p.m.off = ms->off;
    p.m.N = final ? (int)pl.N : 1 << 30;
    p.m.lead = (int)stg.s.lead; p.m.H = H; p.m.depth = ms->mp.depth; p.m.Wa = ms->mp.attack; p.m.Wr = ms->mp.release;
    p.m.f_in = (int)std::min(ms->mp.fade_in, (int64_t)chain::ML_MAX_FADE);
    p.m.f_out = final ? (int)std::min(ms->mp.fade_out, (int64_t)chain::ML_MAX_FADE) : 0;
    p.m.loop = ms->mp.loop; p.m.thr = ms->mp.threshold;
    p.pin = ms->prog[stg.par]; p.pout = ms->prog[w]; p.cin = ms->mc[stg.par]; p.cout = ms->mc[w];
    p.y = s->ml_y; p.need = ms->need; p.L = ms->L; p.out = ms->out;
    p.F0 = (int)F0; p.F1 = (int)pl.F; p.cb0 = (int)stg.base; p.cb1 = (int)pl.base;
    p.h0 = (int)stg.hops; p.h1 = (int)pl.hops; p.kd0 = (int)stg.ducks; p.kd1 = (int)pl.ducks;
    p.q0 = (int)stg.mixed; p.q1 = (int)pl.mixed; p.kl0 = (int)stg.limits; p.kl1 = (int)pl.limits;
    p.out0 = (int)stg.done; p.out1 = (int)pl.done;
    p.mend1 = (int)mend1;
    p.Nend = final ? (int)pl.N : 1 << 30;
    p.xb = p.F0 & ~3; p.pib = p.cb0 & ~3; p.pob = p.cb1 & ~3; p.mb = (int)mend0 & ~3; p.cib = p.out0 & ~3; p.cob = p.out1 & ~3;
    p.cf = (float)chain::lv_ceiling();
    return p;
}

// One push (s->mu held; `pans`: a stereo stream's, the push's own regions, judged behind n).  Everything is judged first;
// the stream's counters move only when the launches went through.
static ft_status ml_push(ft_ctx* ctx, const std::string& fn, ft_mix_stream* ms, const float* x, int64_t n, const chain::MsTable* pans,
                         bool final, float* y, int64_t capacity, int64_t* n_out) {
    CodecState* s = ctx->codec;
    chain::MlStage& stg = ms->st;
    if (stg.ended) return ft_fail(ctx, FT_ERR_STATE, fn + ": the stream has had its final push");
    if (n < 0 || (!x && n > 0) || !n_out) return ft_fail(ctx, FT_ERR_ARG, fn + ": bad argument");
    if (pans)
        if (const char* why = chain::mls_check(*pans, n)) return ft_fail(ctx, FT_ERR_ARG, fn + ": " + why);
    if (n > chain::MX_MAX_N || stg.s.lead + stg.nin + n + stg.s.tail > chain::MX_MAX_N)
        return ft_fail(ctx, FT_ERR_TOO_LONG, fn + ": lead + n + tail exceeds 2^28 samples");
    const chain::MlPlan pl = stg.plan(n, final);
    if (capacity < pl.out || (!y && pl.out > 0)) return ft_fail(ctx, FT_ERR_ARG, fn + ": capacity below what the push emits");
    const int w = stg.par ^ 1, ch = pans ? 2 : 1, R = pans ? (int)pans->R : 0;
    const chain::MlsSizes z = chain::mls_sizes(stg, pl, ch);
    const long long mend1 = final ? pl.N : pl.mixed * stg.s.H;
    hipStream_t st = s->stream;
    FT_TRY(ml_hops(ctx, ms, (size_t)pl.hops + 1));
    FT_TRY(ml_carry(ctx, ms, &ms->prog[w], &ms->pcap[w], z.prog));
    FT_TRY(ml_carry(ctx, ms, &ms->mc[w], &ms->mcap[w], z.mc));
    FT_TRY(cgrow(ctx, &s->ml_x, &s->ml_xcap, z.x));
    FT_TRY(cgrow(ctx, &s->ml_m, &s->ml_mcap, z.m));
    FT_TRY(cgrow(ctx, &s->ml_y, &s->ml_ycap, z.y));
    if (pans) {
        FT_TRY(ml_carry(ctx, ms, &ms->pq[w], &ms->qcap[w], z.pans));
        FT_TRY(cgrow(ctx, &s->ml_q, &s->ml_qcap, z.q));
        FT_TRY(cgrow(ctx, &s->mx_reg, &s->mx_regcap, (size_t)std::max(R, 1)));
    }
    MixLiveSP sp;                                     // (the mono kernels take its MixLiveP alone)
    memset(&sp, 0, sizeof sp);
    sp.l = ml_fill(s, ms, pl, final);
    const MixLiveP& p = sp.l;
    if (n > 0) FT_HIP(ctx, hipMemcpyAsync(s->ml_x + (p.F0 - p.xb), x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    if (pans) {
        sp.bed1 = ms->bed1; sp.U = s->mx_U; sp.reg = s->mx_reg; sp.qx = s->ml_q; sp.qin = ms->pq[stg.par]; sp.qout = ms->pq[w];
        sp.R = R; sp.words = (int)chain::mls_words(p.F0, n);
        if (R > 0) FT_HIP(ctx, hipMemcpyAsync(s->mx_reg, pans->reg, (size_t)R * sizeof(MixPan), hipMemcpyHostToDevice, st));
    }
    const int W = MX_THREADS / 64;
    if (p.h1 > p.h0) mixl_hop_kernel<<<(unsigned)((p.h1 - p.h0 + W - 1) / W), MX_THREADS, 0, st>>>(p);
    if (p.kd1 > p.kd0) mixl_node_kernel<<<(unsigned)((p.kd1 - p.kd0 + MX_THREADS - 1) / MX_THREADS), MX_THREADS, 0, st>>>(p);
    if (sp.words > 0) mixls_pan_kernel<<<(unsigned)((sp.words + MX_THREADS - 1) / MX_THREADS), MX_THREADS, 0, st>>>(sp);
    if (p.q1 > p.q0) {
        if (pans) mixls_sample_kernel<<<(unsigned)(p.q1 - p.q0), MX_THREADS, 0, st>>>(sp);
        else mixl_sample_kernel<<<(unsigned)(p.q1 - p.q0), MX_THREADS, 0, st>>>(p);
    }
    if (p.kl1 > p.kl0) mixl_limit_kernel<<<(unsigned)((p.kl1 - p.kl0 + MX_THREADS - 1) / MX_THREADS), MX_THREADS, 0, st>>>(p);
    // (a lane of the stereo apply kernel writes two frames of the output)
    const long long work = std::max((long long)(pans ? (pl.out + 1) / 2 : pl.out), std::max(mend1 - pl.done, pl.F - pl.base));
    if (work > 0) {
        const unsigned gx = (unsigned)std::min(4096LL, (work + MX_THREADS - 1) / MX_THREADS);
        if (pans) mixls_apply_kernel<<<gx, MX_THREADS, 0, st>>>(sp);
        else mixl_apply_kernel<<<gx, MX_THREADS, 0, st>>>(p);
    }
    if (pl.out > 0) FT_HIP(ctx, hipMemcpyAsync(y, s->ml_y, (size_t)pl.out * ch * sizeof(float), hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, fn + " launch: " + hipGetErrorString(e));
    stg.commit(pl);
    *n_out = pl.out;
    return FT_OK;
}

// The live stage on a whole programme (ft_codec_mix_live; with `pans`, ft_codec_mix_live_stereo): a stream begun, one final
// push, its report and its D and L nodes read back, the stream ended.  The entry point has judged its pointers.
static ft_status ml_live(ft_ctx* ctx, const std::string& fn, const float* x, int64_t n, int rate, const chain::MsTable* pans,
                         const ft_intake_item* bed, const ft_mix_params* mp, float* y, int64_t capacity, int64_t* total,
                         int32_t* duck, int32_t* limit, ft_mix_live_info* info) {
    FT_TRY(mix_refuse(ctx, fn, rate, n, mp, 0, pans));
    const chain::MlPlan pl = chain::ml_plan(ml_shape(rate, mp), n, true);
    if (capacity < pl.N) return ft_fail(ctx, FT_ERR_ARG, fn + ": capacity below lead + n + tail");
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    ft_mix_stream* ms = nullptr;
    FT_TRY(ml_begin(ctx, fn, rate, bed, mp, pans != nullptr, &ms));
    int64_t got = 0;
    ft_status r = ml_push(ctx, fn, ms, x, n, pans, true, y, capacity, &got);
    MixLiveOut out;
    memset(&out, 0, sizeof out);
    hipError_t e = hipSuccess;
    if (r == FT_OK) {
        const size_t nn = (size_t)pl.hops + 1;
        hipStream_t st = s->stream;
        e = hipMemcpyAsync(&out, ms->out, sizeof out, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && duck) e = hipMemcpyAsync(duck, ms->D, nn * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && limit) e = hipMemcpyAsync(limit, ms->L, nn * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) r = ft_fail(ctx, FT_ERR_HIP, fn + ": " + hipGetErrorString(e));
    }
    const long long nb = ms->nb;
    const ft_intake_info binfo = ms->binfo;
    ml_end(ctx, ms);
    FT_TRY(r);
    *total = got;
    memset(info, 0, sizeof *info);
    info->N = pl.N; info->nb = nb; info->Nh = pl.hops; info->active = out.active;
    info->dmax = out.dmax; info->lmax = out.lmax;
    memcpy(&info->qmax, &out.qmax, sizeof(float));
    info->bed = binfo;
    return FT_OK;
}

extern "C" ft_status ft_codec_mix_stream_begin(ft_ctx* ctx, int32_t sample_rate, const ft_intake_item* bed, const ft_mix_params* mp,
                                               ft_mix_stream** out) {
    const std::string fn = "ft_codec_mix_stream_begin";
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!bed || !mp || !out) return ft_fail(ctx, FT_ERR_ARG, fn + ": a null pointer");
    FT_TRY(mix_refuse(ctx, fn, sample_rate, 0, mp, 0, nullptr));
    std::lock_guard<std::mutex> lock(ctx->codec->mu);
    return ml_begin(ctx, fn, sample_rate, bed, mp, false, out);
}

extern "C" ft_status ft_codec_mix_stream_begin_bare(ft_ctx* ctx, int32_t sample_rate, const ft_mix_params* mp, ft_mix_stream** out) {
    const std::string fn = "ft_codec_mix_stream_begin_bare";
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!mp || !out) return ft_fail(ctx, FT_ERR_ARG, fn + ": a null pointer");
    FT_TRY(mix_refuse(ctx, fn, sample_rate, 0, mp, 0, nullptr));
    std::lock_guard<std::mutex> lock(ctx->codec->mu);
    return ml_begin(ctx, fn, sample_rate, nullptr, mp, false, out);
}

extern "C" ft_status ft_codec_mix_stream_begin_stereo(ft_ctx* ctx, int32_t sample_rate, const ft_intake_item* bed,
                                                      const ft_mix_params* mp, ft_mix_stream** out) {
    const std::string fn = "ft_codec_mix_stream_begin_stereo";
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!mp || !out) return ft_fail(ctx, FT_ERR_ARG, fn + ": a null pointer");
    FT_TRY(mix_refuse(ctx, fn, sample_rate, 0, mp, 0, nullptr));
    std::lock_guard<std::mutex> lock(ctx->codec->mu);
    return ml_begin(ctx, fn, sample_rate, bed, mp, true, out);
}

extern "C" ft_status ft_codec_mix_stream_push(ft_mix_stream* ms, const float* x, int64_t n, int32_t final, float* y, int64_t capacity,
                                              int64_t* n_out) {
    if (!ms) return FT_ERR_ARG;
    ft_ctx* ctx = ms->owner;
    if (!ctx || !ctx->codec) return FT_ERR_STATE;      // its context was destroyed
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    if (ms->stereo) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_mix_stream_push: a stereo stream takes ft_codec_mix_stream_push_stereo");
    return ml_push(ctx, "ft_codec_mix_stream_push", ms, x, n, nullptr, final != 0, y, capacity, n_out);
}

extern "C" ft_status ft_codec_mix_stream_push_stereo(ft_mix_stream* ms, const float* x, int64_t n, const ft_pan_region* regions,
                                                     int32_t R, int32_t final, float* y, int64_t capacity, int64_t* n_out) {
    if (!ms) return FT_ERR_ARG;
    ft_ctx* ctx = ms->owner;
    if (!ctx || !ctx->codec) return FT_ERR_STATE;      // its context was destroyed
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    if (!ms->stereo) return ft_fail(ctx, FT_ERR_STATE, "ft_codec_mix_stream_push_stereo: a mono stream takes ft_codec_mix_stream_push");
    const chain::MsTable pans = {(const chain::MsRegion*)regions, R};
    return ml_push(ctx, "ft_codec_mix_stream_push_stereo", ms, x, n, &pans, final != 0, y, capacity, n_out);
}

extern "C" void ft_codec_mix_stream_end(ft_mix_stream* ms) {
    if (!ms) return;
    ft_ctx* own = ms->owner;
    if (own && own->codec) {
        std::lock_guard<std::mutex> lock(own->codec->mu);
        hipSetDevice(own->device);
        ml_end(own, ms);
        return;
    }
    delete ms;
}

extern "C" ft_status ft_codec_mix_live(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_intake_item* bed,
                                       const ft_mix_params* mp, float* y, int64_t capacity, int64_t* total, int32_t* duck,
                                       int32_t* limit, ft_mix_live_info* info) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if ((!x && n != 0) || !bed || !mp || !y || !total || !info) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_mix_live: a null pointer");
    return ml_live(ctx, "ft_codec_mix_live", x, n, sample_rate, nullptr, bed, mp, y, capacity, total, duck, limit, info);
}

extern "C" ft_status ft_codec_mix_live_stereo(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_pan_region* regions,
                                              int32_t R, const ft_intake_item* bed, const ft_mix_params* mp, float* y,
                                              int64_t capacity, int64_t* total, int32_t* duck, int32_t* limit, ft_mix_live_info* info) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if ((!x && n != 0) || !mp || !y || !total || !info) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_mix_live_stereo: a null pointer");
    const chain::MsTable pans = {(const chain::MsRegion*)regions, R};
    return ml_live(ctx, "ft_codec_mix_live_stereo", x, n, sample_rate, &pans, bed, mp, y, capacity, total, duck, limit, info);
}

// ---- live room stage (fishtts_hip.h: "Live room"; rooml_*_kernel in room_kernels.h; the counters, the carry's bounds, the
// per-push checks and the sizes in fx_chain.h, the rl_* block).  A stream owns hn, its RoomOut and two copies of its carry, all
// allocated at `begin` and bounded by predelay + L - 1; a push stages its samples, their sent form and its outputs in the
// context's buffers (the live mix stage's ml_x and ml_y, the room stage's rm_xs) and ends with one wait, so nothing of a push
// outlives it, and the counters move only when the launches went through.
struct ft_room_stream {
    ft_ctx* owner = nullptr;          // null once its context is gone (the device state went with it)
    chain::RlStage st;
    ft_room_params rp;
    int rate = RS_FI;
    long long nh = 0, L = 0;
    float* hn = nullptr;              // [L], for the life of the stream
    float* carry[2] = {nullptr, nullptr};
    RoomOut* out = nullptr;           // E and gn from `begin`, the peak over the pushes so far
    ft_intake_info irinfo;
    std::vector<void*> owned;
};

static void room_stream_orphan(ft_room_stream* rs) {
    for (void* v : rs->owned) hipFree(v);
    rs->owned.clear();
    rs->owner = nullptr;
}

template <typename T>
static ft_status rl_malloc(ft_ctx* ctx, ft_room_stream* rs, T** p, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (n + 8) * sizeof(T));
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_NOMEM, std::string("room stream hipMalloc: ") + hipGetErrorString(e));
    rs->owned.push_back(q);
    *p = (T*)q;
    return FT_OK;
}

static void rl_end(ft_ctx* ctx, ft_room_stream* rs) {   // (s->mu held)
    CodecState* s = ctx->codec;
    hipStreamSynchronize(s->stream);
    for (void* v : rs->owned) hipFree(v);
    rs->owned.clear();
    for (size_t i = 0; i < s->room_streams.size(); ++i)
        if (s->room_streams[i] == rs) { s->room_streams.erase(s->room_streams.begin() + (long)i); break; }
    delete rs;
}

// The stream of a call whose values rm_check has passed (s->mu held): the response prepared as ft_codec_room prepares it, t
// and the block energies in the context's buffers, hn in the stream's own.  A begin that fails once the stream exists frees it.
static ft_status rl_begin(ft_ctx* ctx, const std::string& fn, int rate, const ft_intake_item* ir, const ft_room_params* rp,
                          const chain::RmArgs& a, const chain::RmPlan& pl, ft_room_stream** out) {
    CodecState* s = ctx->codec;
    FxDesc d;
    FT_TRY(fx_refuse(ctx, fn, rate, 100, 0, &d));
    FT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = s->stream;
    ft_mix_params mp;
    memset(&mp, 0, sizeof mp);
    mp.channel = rp->channel;
    MixBed b;                                         // (alive until the wait below)
    FT_TRY(mix_bed(ctx, fn, rate, ir, &mp, false, nullptr, &b));
    if (b.nb != pl.nh) return ft_fail(ctx, FT_ERR_STATE, fn + ": the impulse response's length is not the planned one");
    FT_TRY(mix_table(ctx));
    const chain::RmSizes z = chain::rm_sizes(a, pl);
    FT_TRY(cgrow(ctx, &s->rm_t, &s->rm_tcap, z.taps));
    FT_TRY(cgrow(ctx, &s->rm_e, &s->rm_ecap, z.blocks));
    ft_room_stream* rs = new ft_room_stream();
    rs->owner = ctx;
    rs->rp = *rp;
    rs->rate = rate;
    rs->nh = pl.nh;
    rs->L = pl.L;
    rs->st = chain::RlStage::fresh(chain::rl_shape(a, pl));
    rs->irinfo = b.info;
    s->room_streams.push_back(rs);
    const size_t cz = chain::rl_sizes(rs->st, rs->st.plan(0, false)).carry;
    ft_status r = rl_malloc(ctx, rs, &rs->hn, z.taps);
    if (r == FT_OK) r = rl_malloc(ctx, rs, &rs->out, (size_t)1);
    for (int c = 0; c < 2 && r == FT_OK; ++c) r = rl_malloc(ctx, rs, &rs->carry[c], cz);
    RoomOut got;
    memset(&got, 0, sizeof got);
    if (r == FT_OK) {
        hipError_t e = hipMemsetAsync(rs->out, 0, sizeof(RoomOut), st);
        if (e == hipSuccess) {
            RoomIrP ip = {b.side[0], s->rm_t, rs->hn, s->rm_e, rs->out, (int)pl.L, (int)pl.f, rp->normalize, rp->offset};
            room_ir_kernel<<<(unsigned)((z.blocks + 63) / 64), 64, 0, st>>>(ip);
            room_gain_kernel<<<1, 1024, 0, st>>>(ip);
            e = hipMemcpyAsync(&got, rs->out, sizeof got, hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) r = ft_fail(ctx, FT_ERR_HIP, fn + ": " + hipGetErrorString(e));
    }
    if (r == FT_OK && rp->normalize && (!(got.E > 0.0) || !std::isfinite(got.E)))
        r = ft_fail(ctx, FT_ERR_ARG, fn + ": the impulse response's energy is zero or not finite");
    if (r != FT_OK) {
        rl_end(ctx, rs);
        return r;
    }
    *out = rs;
    return FT_OK;
}

// begin's values judged: the pointers, then rm_check's order without n and the regions, a ceiling other than 0 refused where
// rm_check judges the ceiling.
static ft_status rl_judge(ft_ctx* ctx, const std::string& fn, int rate, const ft_intake_item* ir, const ft_room_params* rp,
                          chain::RmArgs* a, chain::RmPlan* pl) {
    *a = chain::rl_begin_args(room_args(rate, 1, ir, rp));
    bool too_long = false;
    if (const char* why = chain::rm_check(*a, chain::MsTable(), &too_long, pl))
        return ft_fail(ctx, too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG, fn + ": " + why);
    return FT_OK;
}

// One push (s->mu held).  Everything is judged first; the stream's counters move only when the launches went through.
static ft_status rl_push(ft_ctx* ctx, const std::string& fn, ft_room_stream* rs, const float* x, int64_t n, const chain::MsTable& regs,
                         bool final, float* y, int64_t capacity, int64_t* n_out) {
    CodecState* s = ctx->codec;
    chain::RlStage& stg = rs->st;
    bool state = false, too_long = false;
    if (!stg.ended && ((!x && n > 0) || !n_out)) return ft_fail(ctx, FT_ERR_ARG, fn + ": bad argument");
    if (const char* why = chain::rl_check(stg, n, regs, final, capacity, &state, &too_long))
        return ft_fail(ctx, state ? FT_ERR_STATE : too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG, fn + ": " + why);
    const chain::RlPlan pl = stg.plan(n, final);
    if (!y && pl.out > 0) return ft_fail(ctx, FT_ERR_ARG, fn + ": capacity below what the push emits");
    const chain::RlSizes z = chain::rl_sizes(stg, pl);
    const int R = (int)regs.R, w = stg.par ^ 1;
    const bool send = R > 0 || rs->rp.send != 0;
    hipStream_t st = s->stream;
    FT_TRY(cgrow(ctx, &s->ml_x, &s->ml_xcap, z.x));
    FT_TRY(cgrow(ctx, &s->ml_y, &s->ml_ycap, z.y));
    if (send) {
        FT_TRY(cgrow(ctx, &s->rm_xs, &s->rm_xscap, z.xs));
        FT_TRY(cgrow(ctx, &s->mx_reg, &s->mx_regcap, (size_t)std::max(R, 1)));
    }
    std::vector<float> T(chain::MX_MAX_DEPTH + 1);
    chain::mx_gains(T.data());
    if (n > 0) FT_HIP(ctx, hipMemcpyAsync(s->ml_x, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    if (send && n > 0) {
        if (R > 0) FT_HIP(ctx, hipMemcpyAsync(s->mx_reg, regs.reg, (size_t)R * sizeof(MixPan), hipMemcpyHostToDevice, st));
        RoomSendP sp = {s->ml_x, s->rm_xs, s->mx_T, s->mx_reg, (int)n, R, rs->rp.send};
        rooml_send_kernel<<<(unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)), 256, 0, st>>>(sp);
    }
    RoomLive src = {rs->carry[stg.par], send ? s->rm_xs : s->ml_x, (int)pl.cb0, (int)pl.F0, (int)pl.F1};
    if (pl.out > 0) {
        RoomConvP cp;
        memset(&cp, 0, sizeof cp);
        cp.x = s->ml_x; cp.hn = rs->hn; cp.y = s->ml_y; cp.out = rs->out;
        cp.n = (int)pl.F1; cp.L = (int)rs->L; cp.predelay = (int)rs->rp.predelay; cp.N = (int)pl.end;
        cp.dry = rs->rp.dry >= 0; cp.gd = cp.dry ? T[rs->rp.dry] : 0.f; cp.gw = T[rs->rp.wet];
        for (long long i0 = pl.F0; i0 < pl.end; i0 += RM_LAUNCH) {
            cp.i0 = (int)i0;
            const long long span = std::min<long long>(RM_LAUNCH, pl.end - i0);
            rooml_conv_kernel<<<(unsigned)((span + RM_SPAN - 1) / RM_SPAN), RM_THREADS, 0, st>>>(cp, src);
        }
    }
    if (pl.F1 > pl.cb1) {
        RoomRollP rp = {src, rs->carry[w], (int)pl.cb1};
        rooml_roll_kernel<<<(unsigned)std::min<long long>(4096, (pl.F1 - pl.cb1 + 255) / 256), 256, 0, st>>>(rp);
    }
    if (pl.out > 0) FT_HIP(ctx, hipMemcpyAsync(y, s->ml_y, (size_t)pl.out * sizeof(float), hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(ctx, FT_ERR_HIP, fn + " launch: " + hipGetErrorString(e));
    stg.commit(pl);
    *n_out = pl.out;
    return FT_OK;
}

static ft_status rl_info(ft_ctx* ctx, const std::string& fn, ft_room_stream* rs, ft_room_info* info) {   // (s->mu held)
    hipStream_t st = ctx->codec->stream;
    RoomOut out;
    FT_HIP(ctx, hipMemcpyAsync(&out, rs->out, sizeof out, hipMemcpyDeviceToHost, st));
    FT_HIP(ctx, hipStreamSynchronize(st));
    (void)fn;
    memset(info, 0, sizeof *info);
    info->N = rs->st.nout; info->nh = rs->nh; info->L = rs->L; info->E = out.E; info->gn = out.gn;
    memcpy(&info->pk, &out.pk, sizeof(float));
    info->sg = 1.f;
    info->capped = 0;
    info->ir = rs->irinfo;
    return FT_OK;
}

extern "C" ft_status ft_codec_room_stream_begin(ft_ctx* ctx, int32_t sample_rate, const ft_intake_item* ir, const ft_room_params* rp,
                                                ft_room_stream** out) {
    const std::string fn = "ft_codec_room_stream_begin";
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if (!ir || !rp || !out) return ft_fail(ctx, FT_ERR_ARG, fn + ": a null pointer");
    chain::RmArgs a;
    chain::RmPlan pl;
    FT_TRY(rl_judge(ctx, fn, sample_rate, ir, rp, &a, &pl));
    std::lock_guard<std::mutex> lock(ctx->codec->mu);
    return rl_begin(ctx, fn, sample_rate, ir, rp, a, pl, out);
}

extern "C" ft_status ft_codec_room_stream_push(ft_room_stream* rs, const float* x, int64_t n, const ft_send_region* regions, int32_t R,
                                               int32_t final, float* y, int64_t capacity, int64_t* n_out) {
    if (!rs) return FT_ERR_ARG;
    ft_ctx* ctx = rs->owner;
    if (!ctx || !ctx->codec) return FT_ERR_STATE;      // its context was destroyed
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    const chain::MsTable regs = {(const chain::MsRegion*)regions, R};
    return rl_push(ctx, "ft_codec_room_stream_push", rs, x, n, regs, final != 0, y, capacity, n_out);
}

extern "C" ft_status ft_codec_room_stream_info(ft_room_stream* rs, ft_room_info* info) {
    if (!rs) return FT_ERR_ARG;
    ft_ctx* ctx = rs->owner;
    if (!ctx || !ctx->codec) return FT_ERR_STATE;      // its context was destroyed
    if (!info) return ft_fail(ctx, FT_ERR_ARG, "ft_codec_room_stream_info: a null pointer");
    std::lock_guard<std::mutex> lock(ctx->codec->mu);
    FT_HIP(ctx, hipSetDevice(ctx->device));
    return rl_info(ctx, "ft_codec_room_stream_info", rs, info);
}

extern "C" void ft_codec_room_stream_end(ft_room_stream* rs) {
    if (!rs) return;
    ft_ctx* own = rs->owner;
    if (own && own->codec) {
        std::lock_guard<std::mutex> lock(own->codec->mu);
        hipSetDevice(own->device);
        rl_end(own, rs);
        return;
    }
    delete rs;
}

// The stage on a whole programme: a stream begun, one final push, its report, the stream ended.
extern "C" ft_status ft_codec_room_live(ft_ctx* ctx, const float* x, int64_t n, int32_t sample_rate, const ft_send_region* regions,
                                        int32_t R, const ft_intake_item* ir, const ft_room_params* rp, float* y, int64_t capacity,
                                        int64_t* total, ft_room_info* info) {
    const std::string fn = "ft_codec_room_live";
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx));
    if ((!x && n != 0) || !ir || !rp || !y || !total || !info) return ft_fail(ctx, FT_ERR_ARG, fn + ": a null pointer");
    chain::RmArgs a;
    chain::RmPlan pl;
    FT_TRY(rl_judge(ctx, fn, sample_rate, ir, rp, &a, &pl));
    const chain::MsTable regs = {(const chain::MsRegion*)regions, R};
    if (pl.nh >= 0) {                                   // (an item the intake refuses has no nh: its refusal stands, in rl_begin)
        bool state = false, too_long = false;
        if (const char* why = chain::rl_check(chain::RlStage::fresh(chain::rl_shape(a, pl)), n, regs, true, capacity, &state, &too_long))
            return ft_fail(ctx, too_long ? FT_ERR_TOO_LONG : FT_ERR_ARG, fn + ": " + why);
    }
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    ft_room_stream* rs = nullptr;
    FT_TRY(rl_begin(ctx, fn, sample_rate, ir, rp, a, pl, &rs));
    int64_t got = 0;
    ft_status r = rl_push(ctx, fn, rs, x, n, regs, true, y, capacity, &got);
    if (r == FT_OK) r = rl_info(ctx, fn, rs, info);
    rl_end(ctx, rs);
    FT_TRY(r);
    *total = got;
    return FT_OK;
}

// ---- launch trace hooks (fishtts_hip_test.h)
extern "C" ft_status ft_test_codec_trace_arm(ft_ctx* ctx, int32_t first, int32_t count) {
    if (!ctx) return FT_ERR_ARG;
    FT_TRY(codec_ready(ctx, false));
    if (first < 0 || count < 0) return ft_fail(ctx, FT_ERR_ARG, "ft_test_codec_trace_arm: bad range");
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    s->tstore.recs.clear();
    s->tstore.first = first; s->tstore.count = count; s->tstore.armed = true; s->tstore.failed = false;
    return FT_OK;
}
extern "C" int32_t ft_test_codec_trace_count(ft_ctx* ctx) {
    if (!ctx || !ctx->codec) return -1;
    std::lock_guard<std::mutex> lock(ctx->codec->mu);
    return ctx->codec->tstore.failed ? -1 : (int32_t)ctx->codec->tstore.recs.size();
}
extern "C" ft_status ft_test_codec_trace_chunks(ft_ctx* ctx, int32_t* n, int32_t* table) {
    if (!ctx || !ctx->codec || !n) return FT_ERR_ARG;
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    *n = (int32_t)s->tstore.chunks.size();
    for (size_t z = 0; table && z < s->tstore.chunks.size(); ++z) {
        const CodecState::TraceChunk& c = s->tstore.chunks[z];
        table[4 * z] = c.P; table[4 * z + 1] = c.L; table[4 * z + 2] = c.t0; table[4 * z + 3] = c.nh;
    }
    return FT_OK;
}
extern "C" int32_t ft_test_codec_trace_variants(void) { return N_GEMM_VARIANTS; }
extern "C" const char* ft_test_codec_trace_variant(int32_t id, int32_t* bm, int32_t* bn) {
    if (id < 0 || id >= N_GEMM_VARIANTS) return nullptr;
    if (bm) *bm = GEMM_VARIANTS[id].bm;
    if (bn) *bn = GEMM_VARIANTS[id].bn;
    return GEMM_VARIANTS[id].name;
}
extern "C" ft_status ft_test_codec_trace_launch(ft_ctx* ctx, int32_t i, char* name, int32_t cap, int32_t* info) {
    if (!ctx || !ctx->codec || !name || cap < 1 || !info) return FT_ERR_ARG;
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    if (i < 0 || i >= (int)s->tstore.recs.size()) return ft_fail(ctx, FT_ERR_ARG, "ft_test_codec_trace_launch: no such launch");
    const CodecState::TraceRec& r = s->tstore.recs[i];
    snprintf(name, (size_t)cap, "%s", r.name.c_str());
    info[0] = r.rows; info[1] = r.cols; info[2] = r.variant; info[3] = (int32_t)r.bufs.size();
    info[4] = r.halo; info[5] = r.ntap; info[6] = r.K; info[7] = r.held ? 1 : 0;
    return FT_OK;
}
extern "C" ft_status ft_test_codec_trace_buffer(ft_ctx* ctx, int32_t i, int32_t j, int32_t* kind, int32_t* is_f32, int64_t* elems,
                                                void* dst) {
    if (!ctx || !ctx->codec || !kind || !is_f32 || !elems) return FT_ERR_ARG;
    CodecState* s = ctx->codec;
    std::lock_guard<std::mutex> lock(s->mu);
    if (i < 0 || i >= (int)s->tstore.recs.size() || j < 0 || j >= (int)s->tstore.recs[i].bufs.size())
        return ft_fail(ctx, FT_ERR_ARG, "ft_test_codec_trace_buffer: no such buffer");
    CodecState::TraceBuf& b = s->tstore.recs[i].bufs[j];
    *kind = b.kind; *is_f32 = b.f32; *elems = b.elems;
    if (dst) {
        if (b.data.empty()) return ft_fail(ctx, FT_ERR_STATE, "ft_test_codec_trace_buffer: launch outside the armed range");
        memcpy(dst, b.data.data(), b.data.size());
        std::vector<char>().swap(b.data);   // handed over: a 215-frame stage is tens of MB
    }
    return FT_OK;
}
