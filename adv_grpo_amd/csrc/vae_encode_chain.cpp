// vae_encode_chain.cpp -- the SD3 / SD3.5 VAE encoder (fp32-equivalent arithmetic) behind ONE C-ABI entry, "advgrpo_vae_encode".
//
// Stands in for `pipe.vae.encode(img_tensor)` up to the moments of its latent distribution
// (adv_grpo/diffusers_patch/sd3_pipeline_with_logprob_fast.py:703; the reference runs the VAE in fp32, train_sd3_fast_pickscore.py:481):
// diffusers' AutoencoderKL encoder -- Normalize, conv_in, the down blocks (resnets, then Downsample2D(padding=0) = F.pad(x, (0, 1, 0, 1)) + a 3x3
// convolution of stride 2, folded into that convolution's tap addressing), the mid block (resnet, single-head attention, resnet), GroupNorm +
// SiLU + conv_out to 2 * latent_channels moments.  The launch order of adv_grpo_amd/vae_encoder.py (_moments_chain) in C++, bit-identical to it
// (tests/test_gpu_vae_encoder.py).  Every convolution runs on split-bf16 operands, three products (advgrpo_vae_conv.form 0); everything
// between two matrix products stays f32.  Sampling, scaling and the cast are advgrpo_vae_latent_tail's (vae_encode.hip).
// Host-only code: it only calls this library's own C entries.
#include <algorithm>

#include "common.hpp"
#include "vae_chain.hpp"

using namespace advgrpo;
using vae_chain::piece;

namespace {

constexpr int IMG_CPAD = 64;                 // the 3 image channels padded to one 64-channel slice of the convolution kernel

struct Plan {
    int64_t max_elems = 0;                   // largest f32 activation [B, H, W, C]
    int64_t max_rows = 0;                    // largest convolution input (operand rows: 6 bytes per element)
    int64_t gn_scratch = 0;
    int64_t attn = 0;                        // the mid attention's scratch, score matrix included
    int64_t slot_bytes() const { return piece(max_elems * 4); }
    int64_t rows_bytes() const { return piece(max_rows * 6); }
    int64_t total() const { return 3 * slot_bytes() + rows_bytes() + piece(gn_scratch) + attn + 256; }
};

bool desc_ok(const advgrpo_vae_decoder_desc* d) {
    return d && d->B > 0 && d->h > 0 && d->w > 0 && d->n_up > 0 && d->n_up <= 8 && d->resnets_per_up > 0 && d->groups > 0 && d->up_resnets &&
           (d->n_up == 1 || d->upsamplers) && d->h % (1 << (d->n_up - 1)) == 0 && d->w % (1 << (d->n_up - 1)) == 0;
}

Plan plan_of(const advgrpo_vae_decoder_desc& d) {
    Plan p;
    const int B = d.B;
    int H = d.h, W = d.w;
    auto see = [&](int c) { p.max_elems = std::max<int64_t>(p.max_elems, (int64_t)B * H * W * c); };
    auto see_in = [&](int c) { p.max_rows = std::max<int64_t>(p.max_rows, (int64_t)B * H * W * c); };
    auto see_gn = [&]() { p.gn_scratch = std::max<int64_t>(p.gn_scratch, advgrpo_groupnorm_scratch_bytes(B, H * W, d.groups)); };
    see_in(IMG_CPAD);
    see(d.conv_in.cout);
    int C = d.conv_in.cout;
    for (int i = 0; i < d.n_up; ++i) {
        for (int j = 0; j < d.resnets_per_up; ++j) {
            const advgrpo_vae_resnet& r = d.up_resnets[i * d.resnets_per_up + j];
            see(r.conv1.cin); see(r.conv1.cout); see(r.conv2.cout);
            see_in(r.conv1.cin); see_in(r.conv2.cin);
            see_gn();
            C = r.conv2.cout;
        }
        if (i < d.n_up - 1) {
            see_in(d.upsamplers[i].cin);
            H /= 2; W /= 2;
            see(d.upsamplers[i].cout);
            C = d.upsamplers[i].cout;
        }
    }
    see(C); see_in(C); see_gn();
    see(std::max(d.conv_out.cout, 4));
    const int64_t T = (int64_t)H * W;
    p.attn = vae_chain::attn_rest_bytes(B, T, C) + vae_chain::attn_s_bytes(B, T);
    return p;
}

}  // namespace

extern "C" int64_t advgrpo_vae_encode_workspace_bytes(const advgrpo_vae_decoder_desc* d) {
    if (!desc_ok(d)) return -1;
    return plan_of(*d).total();
}

extern "C" int advgrpo_vae_encode(const advgrpo_vae_decoder_desc* dsc, const void* images, int images_dtype, float* moments, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    ADVGRPO_CHECK(dsc && images && moments && workspace, "vae_encode: null argument");
    const advgrpo_vae_decoder_desc& d = *dsc;
    ADVGRPO_CHECK(desc_ok(dsc) && d.zero_page && d.conv_in.w && d.conv_in.bias && d.conv_out.w && d.conv_out.bias && d.norm_out_w && d.norm_out_b &&
                      d.attn_norm_w && d.attn_norm_b && d.attn_q_w && d.attn_k_w && d.attn_v_w && d.attn_o_w && d.attn_q_b && d.attn_k_b && d.attn_v_b &&
                      d.attn_o_b,
                  "vae_encode: bad descriptor (B, h, w > 0 with h, w multiples of 2^(n_up - 1); weights, zero page)");
    {
        const int dn = 1 << (d.n_up - 1);
        ADVGRPO_CHECK(((int64_t)(d.h / dn) * (d.w / dn)) % 64 == 0, "vae_encode: the mid attention needs (h / %d) * (w / %d) to be a multiple of 64 (h=%d w=%d)", dn, dn, d.h, d.w);
    }
    ADVGRPO_CHECK(d.conv_in.form == 0 && d.conv_out.form == 0 && d.conv_in.cin == IMG_CPAD && d.conv_in.cout >= 128 && d.conv_out.cout == 2 * d.latent_channels,
                  "vae_encode: conv_in / conv_out run on split-bf16 operands (form 0), conv_in from the image padded to %d channels to >= 128, conv_out to 2 x latent_channels",
                  IMG_CPAD);
    ADVGRPO_CHECK(images_dtype == ADVGRPO_F32 || images_dtype == ADVGRPO_BF16 || images_dtype == ADVGRPO_U8, "vae_encode: images must be f32 / bf16 NCHW or uint8 NHWC");
    auto conv_ok = [](const advgrpo_vae_conv& c) { return c.w && c.bias && c.form == 0 && c.cin > 0 && c.cin % 64 == 0 && c.cout >= 128; };
    auto res_ok = [&](const advgrpo_vae_resnet& r) { return r.norm1_w && r.norm1_b && r.norm2_w && r.norm2_b && conv_ok(r.conv1) && conv_ok(r.conv2) &&
                                                            r.conv1.cout == r.conv2.cin && (r.shortcut_w || r.conv1.cin == r.conv2.cout); };
    {
        bool ok = res_ok(d.mid[0]) && res_ok(d.mid[1]);
        for (int i = 0; i < d.n_up * d.resnets_per_up; ++i) ok = ok && res_ok(d.up_resnets[i]);
        for (int i = 0; i + 1 < d.n_up; ++i) ok = ok && conv_ok(d.upsamplers[i]);
        ADVGRPO_CHECK(ok, "vae_encode: every resnet / downsampler convolution needs weights, form 0 (split-bf16), cin a multiple of 64 and cout >= 128");
    }
    ADVGRPO_CHECK(workspace_bytes >= advgrpo_vae_encode_workspace_bytes(dsc) && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                  "vae_encode: workspace too small or not 256-byte aligned");
    const Plan plan = plan_of(d);
    const int B = d.B, G = d.groups;
    char* w = reinterpret_cast<char*>(workspace);
    auto take = [&](int64_t bytes) { char* p = w; w += piece(bytes); return p; };
    float* act[3] = {reinterpret_cast<float*>(take(plan.slot_bytes())), reinterpret_cast<float*>(take(plan.slot_bytes())),
                     reinterpret_cast<float*>(take(plan.slot_bytes()))};
    char* rows = take(plan.rows_bytes());
    double* gn = reinterpret_cast<double*>(take(plan.gn_scratch));
    char* attn = take(plan.attn);
    int rc;
    int H = d.h, W = d.w;
    auto other = [&](int a, int b) { for (int s = 0; s < 3; ++s) if (s != a && s != b) return s; return 0; };
    // 3x3 convolution of SiLU(GroupNorm(act[xs])) (+ residual) into `out`
    auto conv_gn = [&](const advgrpo_vae_conv& c, const float* nw, const float* nb, int xs, const float* residual, float* out) -> int {
        if ((rc = advgrpo_groupnorm_nhwc_x3(act[xs], rows, gn, nw, nb, B, H * W, c.cin, G, 1e-6f, 1, c.cout >= 128 ? 1 : 0, stream)) != 0) return rc;
        return advgrpo_conv3x3_nhwc_x3(rows, c.w, out, B, H, W, 3 * c.cin, c.cout, 0, c.bias, 0, residual, d.zero_page, stream);
    };
    // ResnetBlock2D: x -> conv1(SiLU(GN(x))) -> conv2(SiLU(GN(.))) + shortcut(x) (the 1x1 shortcut's bias rides on conv2's)
    auto resnet = [&](const advgrpo_vae_resnet& r, int& xs) -> int {
        const int hs = (xs + 1) % 3, ss = other(xs, hs);
        if ((rc = conv_gn(r.conv1, r.norm1_w, r.norm1_b, xs, nullptr, act[hs])) != 0) return rc;
        const float* sc = act[xs];
        if (r.shortcut_w) {
            const int64_t M = (int64_t)B * H * W;
            if ((rc = advgrpo_split_bf16x3(act[xs], nullptr, rows, M, r.conv1.cin, 0, stream)) != 0) return rc;
            if ((rc = advgrpo_gemm_bf16(rows, 3 * r.conv1.cin, r.shortcut_w, 3 * r.conv1.cin, act[ss], r.conv2.cout, ADVGRPO_F32, (int)M, r.conv2.cout, 3 * r.conv1.cin,
                                        nullptr, 0, 1.0f, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, stream)) != 0)
                return rc;
            sc = act[ss];
        }
        if ((rc = conv_gn(r.conv2, r.norm2_w, r.norm2_b, hs, sc, act[hs])) != 0) return rc;
        xs = hs;
        return 0;
    };

    // ---- Normalize + conv_in
    if ((rc = advgrpo_image_to_nhwc_x3(images, images_dtype, rows, B, H, W, IMG_CPAD, stream)) != 0) return rc;
    if ((rc = advgrpo_conv3x3_nhwc_x3(rows, d.conv_in.w, act[0], B, H, W, 3 * IMG_CPAD, d.conv_in.cout, 0, d.conv_in.bias, 0, nullptr, d.zero_page, stream)) != 0) return rc;
    int xs = 0;
    // ---- down blocks
    for (int i = 0; i < d.n_up; ++i) {
        for (int j = 0; j < d.resnets_per_up; ++j)
            if ((rc = resnet(d.up_resnets[i * d.resnets_per_up + j], xs)) != 0) return rc;
        if (i < d.n_up - 1) {
            const advgrpo_vae_conv& dn = d.upsamplers[i];
            const int os = (xs + 1) % 3;
            if ((rc = advgrpo_split_bf16x3(act[xs], nullptr, rows, (int64_t)B * H * W, dn.cin, 2, stream)) != 0) return rc;
            H /= 2; W /= 2;
            if ((rc = advgrpo_conv3x3_s2_nhwc_x3(rows, dn.w, act[os], B, H, W, 3 * dn.cin, dn.cout, dn.bias, d.zero_page, stream)) != 0) return rc;
            xs = os;
        }
    }
    // ---- mid block
    if ((rc = resnet(d.mid[0], xs)) != 0) return rc;
    {
        const int ns = (xs + 1) % 3;
        if ((rc = vae_chain::vae_mid_attention(d, B, H, W, d.mid[0].conv2.cout, act[xs], act[ns], attn, nullptr, gn, stream)) != 0) return rc;
        xs = ns;
    }
    if ((rc = resnet(d.mid[1], xs)) != 0) return rc;
    // ---- conv_norm_out + SiLU + conv_out
    const int cl = d.conv_out.cin;
    if ((rc = advgrpo_groupnorm_nhwc_x3(act[xs], rows, gn, d.norm_out_w, d.norm_out_b, B, H * W, cl, G, 1e-6f, 1, d.conv_out.cout >= 128 ? 1 : 0, stream)) != 0) return rc;
    return advgrpo_conv3x3_nhwc_x3(rows, d.conv_out.w, moments, B, H, W, 3 * cl, d.conv_out.cout, 0, d.conv_out.bias, 0, nullptr, d.zero_page, stream);
}
