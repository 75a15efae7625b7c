// Host side shared by the reduced-multiply kernels (conv_wino.hip, convt_wino.hip, conv1d_wino.hip, conv_wino44{,s,w}.hip): descriptor
// checks and the packer of the standard weight-stream order (launch_lds_ceiling: conv_host.h, shared with the direct kernels).
// What differs between the kernels stays at their call sites: this header makes none of them behave like another.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/monorec_hip.h"
#include "conv_host.h"
#include "cooktoom_1d.h"

static inline int pad8(int c) { return (c + 7) & ~7; }

// K chunks of `ck` input channels over the concatenated sources (a chunk never straddles two sources)
static inline int wino_chunks(const int32_t* src_channels, int num_src, int ck = 8) {
    int n = 0;
    for (int s = 0; s < num_src; ++s) n += mr_ceil_div(src_channels[s], ck);
    return n;
}

static inline int wino_sum_channels(const int32_t* src_channels, int num_src) {
    int c = 0;
    for (int s = 0; s < num_src; ++s) c += src_channels[s];
    return c;
}

// G of F(2, 3) (points 0, +-1, infinity): the 1-D kernels use G g, the F(2x2, 3x3) kernel G g G^T
static const double WINO_G_2_3[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};

// U[pi][pj] of F(4x4, 3x3) = (G g G^T)[pi][pj] for one 3x3 filter `gw`, G of F(4, 3) (cooktoom_1d.h), in double
static inline double wino_u44(const float* gw, int pi, int pj) {
    double u = 0.0;
    for (int i = 0; i < 3; ++i) {
        double row = 0.0;
        for (int j = 0; j < 3; ++j) row += (double)gw[i * 3 + j] * CT_G_4_3[pj][j];
        u += CT_G_4_3[pi][i] * row;
    }
    return u;
}

// ---- descriptor checks: the tests every derive* function opens with, in three pieces because the entry points order them differently
static inline int wino_check_shape(const mr_wino_desc* d) {
    if (!d || d->num_src < 1 || d->num_src > MR_MAX_SOURCES || d->batch < 1 || d->height < 1 || d->width < 4 || !d->dst ||
        !d->packed_weights || d->out_channels < 1)
        return MR_ERR_BAD_ARGUMENT;
    return d->width % 4 ? MR_ERR_UNSUPPORTED : 0;             // 16-byte groups entirely inside or outside the image
}
static inline int wino_check_activation(const mr_wino_desc* d) {
    if (d->activation != MR_ACT_NONE && d->activation != MR_ACT_RELU && d->activation != MR_ACT_LEAKY_RELU) return MR_ERR_UNSUPPORTED;
    if (d->activation == MR_ACT_LEAKY_RELU && !(d->act_p0 >= 0.f && d->act_p0 <= 1.f)) return MR_ERR_UNSUPPORTED;   // the epilogue is max(x, x * slope)
    return 0;
}
// strided source views / a parity-split destination: mr_conv1d_cooktoom_f32 only
static inline bool wino_is_view(const mr_wino_desc* d) { return d->src_row_pitch || d->src_plane_floats || d->dst_split_columns; }

static inline long long wino_dst_bytes(const mr_wino_desc* d) { return (long long)d->batch * d->out_channels * d->height * d->width * 4; }

// Clears `k`, then fills its sources (channels padded to chunks of `ck`) and the scalar fields every kernel-args struct has; returns the
// chunk count through `nchunks`.  A source spans batch * channels planes of `plane_floats` floats, less the `view_slack` floats that a view
// starting inside its tensor leaves behind (dense: height * width and 0), and must stay below 2^31 bytes (32-bit offsets of the descriptor).
template <class K>
int wino_fill_args(const mr_wino_desc* d, int ck, long long plane_floats, int view_slack, K& k, int& nchunks) {
    memset(&k, 0, sizeof(k));
    nchunks = 0;
    for (int s = 0; s < d->num_src; ++s) {
        if (!d->src[s] || d->src_channels[s] < 1) return MR_ERR_BAD_ARGUMENT;
        const long long bytes = ((long long)d->batch * d->src_channels[s] * plane_floats - view_slack) * 4;
        if (bytes >= (1ll << 31) || bytes <= 0) return MR_ERR_UNSUPPORTED;
        k.src[s] = d->src[s];
        k.src_bytes[s] = (int)bytes;
        k.src_c[s] = d->src_channels[s];
        k.src_cpad[s] = mr_ceil_div(d->src_channels[s], ck) * ck;
        nchunks += k.src_cpad[s] / ck;
    }
    k.nsrc = d->num_src;
    k.H = d->height; k.W = d->width;
    k.dst = d->dst; k.bias = d->bias;
    k.act = d->activation; k.p0 = d->act_p0;
    k.Cout = d->out_channels;
    k.w = d->packed_weights;
    return 0;
}

// One weight stream in the standard order: [cout group of `blocks` 16-channel blocks][source][chunk of 8 channels][position < npos]
// [channel quad][cout block][64 lanes], lane l = (cout l & 15 of the block, channel l >> 4 of the quad), each chunk followed by `chunk_pad`
// zeros.  Covers the output channels cout_begin .. cout_end - 1; u(cout, cin, position) is the transformed weight in double (rounded to
// fp32 here, once), cin counted over the concatenated sources; padded channels and output channels are zero.  Returns the floats written.
template <class U>
size_t wino_pack_stream(float* dst, int cout_begin, int cout_end, int blocks, int npos, int chunk_pad, const int32_t* src_channels,
                        int num_src, U u) {
    const int groups = mr_ceil_div(cout_end - cout_begin, 16 * blocks);
    size_t o = 0;
    for (int g = 0; g < groups; ++g) {
        int cin_off = 0;
        for (int s = 0; s < num_src; ++s) {
            for (int c0 = 0; c0 < pad8(src_channels[s]); c0 += 8) {
                for (int p = 0; p < npos; ++p)
                    for (int c4 = 0; c4 < 2; ++c4)
                        for (int mb = 0; mb < blocks; ++mb)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int cout = cout_begin + (g * blocks + mb) * 16 + (lane & 15);
                                const int cl = c0 + c4 * 4 + (lane >> 4);
                                dst[o++] = cout < cout_end && cl < src_channels[s] ? (float)u(cout, cin_off + cl, p) : 0.f;
                            }
                for (int z = 0; z < chunk_pad; ++z) dst[o++] = 0.f;
            }
            cin_off += src_channels[s];
        }
    }
    return o;
}
