/*
 * monorec_hip.h - C ABI of libmonorec_hip.so: the MI355X (gfx950) kernels behind the MonoRec
 * cost-volume inference path.
 *
 * The reference (Brummi/MonoRec) is pure Python on PyTorch; its "FFI" for this path is the set of
 * ATen operator calls inside MonoRecModel.forward.  Each entry point below replaces one group of
 * those calls; the comment on every function names the reference lines it stands in for
 * (paths relative to the reference root).
 *
 * Conventions
 *   - plain C: raw device pointers, ints/floats and a `void* stream` (a hipStream_t); no torch types.
 *   - the caller owns every buffer; all tensors are dense fp32 NCHW on the current HIP device.
 *   - every launch is asynchronous on `stream`; nothing here allocates, frees or synchronises,
 *     so all entry points may be recorded into a hipGraph (stream capture).
 *   - return value: 0 on success, a positive hipError_t, or a negative MR_ERR_* code. Nothing throws
 *     across the boundary. mr_error_string() maps a code to text.
 *   - this file is the only statement of the ABI: the Python binding (monorec_amd/_lib.py) reads it at import and builds its ctypes
 *     prototypes, structs and constants from it.  It reads these forms, and anything else at top level makes the import raise:
 *       #define MR_NAME <integer expression over decimal / hex literals, + - * ( ) and earlier MR_ names>, also inside an
 *         #ifndef MR_NAME ... #endif that gives a default;
 *       enum { MR_NAME = <such an expression>, ... };
 *       typedef struct [tag] { <type> name[, name...]; ... } mr_...;  fields scalar, pointer or array of <such an expression>;
 *       <type> mr_...(<type> name, ...);  or (void);  what stands in #ifdef MR_DIAGNOSTIC_LIBRARY is typed when exported, not required.
 *     <type> is int, int32_t, int64_t, float, double, size_t, a pointer (to those, to void, char or a fixed-width integer, to a
 *     pointer, or to a struct declared earlier here), and const char* for a return value.  A struct the host fills carries its name as
 *     the tag and the binding takes a typed pointer to it; a struct the device fills (mr_median_stats) is declared without a tag, and a
 *     pointer to it is a device address like every other pointer.
 */
#ifndef MONOREC_HIP_H
#define MONOREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MR_ABI_VERSION 24

#define MR_COMPUTE_F32  0
#define MR_COMPUTE_BF16 1
#define MR_COMPUTE_BF16X3 2

#define MR_ERR_BAD_ARGUMENT (-1)
#define MR_ERR_UNSUPPORTED  (-2)
#define MR_ERR_LDS_BUDGET   (-3)

#define MR_MAX_SOURCES 3
#define MR_MAX_FRAMES  8
#define MR_MAX_HEADS   4   /* one-channel 3x3 heads per mr_depth_heads_f32 launch (DepthModule has 4 predictors) */
#define MR_MAX_VOTE_MASKS 8   /* masks voted over by mr_pointcloud_append_f32 / mr_tsdf_frame_f32 (the reference buffers 5) */
#define MR_TSDF_MAX_FRAMES 8  /* keyframes integrated by one mr_tsdf_integrate_f32 launch */
#define MR_CONSISTENCY_MAX_VIEWS 8   /* neighbouring keyframes checked by one mr_depth_consistency_f32 launch */
#define MR_TSDF_TILE_X 32     /* voxels of one workgroup of mr_tsdf_integrate_f32 - the unit of its frustum culling */
#define MR_TSDF_TILE_Y 8
#define MR_TSDF_TILE_Z 4
#define MR_TSDF_BLOCK 8       /* edge, in voxels, of one block of the block-sparse volume (mr_tsdf_sparse_*_f32) */
#ifndef MR_TSDF_BRICK         /* (a build with -DMR_TSDF_BRICK=8 exists for tools/bench_tsdf_render.py --brick 8 alone) */
#define MR_TSDF_BRICK 4       /* edge, in voxels, of one brick of mr_tsdf_skip_grid_u8: 4 or 8, 4 by measurement */
#endif

/* ---- activation codes for mr_conv2d_f32 (epilogue, applied after bias [+ residual]) ---- */
enum {
    MR_ACT_NONE = 0,
    MR_ACT_RELU = 1,            /* torchvision BasicBlock relu                                   */
    MR_ACT_LEAKY_RELU = 2,      /* LeakyReLU(slope = act_p0), 0 <= act_p0 <= 1 (else MR_ERR_UNSUPPORTED)  model/layers.py:303,330,391 */
    MR_ACT_SIGMOID = 3,         /* MaskModule.classifier      model/monorec/monorec_model.py:342  */
    MR_ACT_ABS_TANH_AFFINE = 4  /* |tanh(x)| then (1-p)*act_p0 + p*act_p1  monorec_model.py:556,717 */
};

/* ---- how the conv reads its (virtual) input plane from the stored source plane ---- */
enum {
    MR_IN_DIRECT = 0,     /* input == source                                                          */
    MR_IN_UPSAMPLE2 = 1,  /* input(y,x) = source(y/2,x/2): nn.Upsample(scale_factor=2) layers.py:349   */
    MR_IN_MAXPOOL2 = 2    /* input(y,x) = max of the 2x2 source block: nn.MaxPool2d(2) monorec_model.py:304 */
};

/* ---- value transform applied to in-bounds input samples while staging ---- */
enum {
    MR_TF_NONE = 0,
    MR_TF_RESNET_NORM = 1 /* ((x + 0.5) - 0.45) / 0.225  monorec_model.py:691 + :120 */
};

/*
 * One convolution launch.  Replaces nn.Conv2d / PadSameConv2d+Conv2d / Upsample+pad+Conv2d /
 * MaxPool2d+Conv2d / one output phase of ConvTranspose2d(k4,s2) (+ folded eval BatchNorm, bias,
 * residual add and activation) of model/layers.py:241-252,289-356,380-400 and the torchvision
 * ResNet-18 trunk used by model/monorec/monorec_model.py:118-129.
 *
 * Input = channel concatenation (torch.cat(..., dim=1), monorec_model.py:372-380,531,541-545) of
 * `num_src` NCHW sources sharing batch and plane size; they are read in place, never materialised.
 * Output pixel (oy,ox) of the conv grid is written to plane position
 * (oy*out_step_h + out_off_h, ox*out_step_w + out_off_w) of channel dst_channel_offset + co of a
 * (batch, dst_total_channels, dst_plane_h, dst_plane_w) tensor - step 2 is used by the four phases of
 * the transposed convolution.
 */
typedef struct mr_conv_desc {
    /* input */
    const float* src[MR_MAX_SOURCES];
    int32_t src_channels[MR_MAX_SOURCES];
    int32_t num_src;
    int32_t batch;
    int32_t src_h, src_w;            /* stored plane size of every source                      */
    int32_t in_mode;                 /* MR_IN_*                                                */
    int32_t in_transform;            /* MR_TF_*                                                */
    /* filter geometry; taps read input (oy*stride_h - pad_top + ky, ox*stride_w - pad_left + kx), zero outside */
    int32_t kh, kw, stride_h, stride_w, pad_top, pad_left;
    int32_t out_h, out_w;            /* conv grid size                                          */
    /* output placement */
    float* dst;
    int32_t out_channels;
    int32_t dst_total_channels, dst_channel_offset;
    int32_t dst_plane_h, dst_plane_w;
    int32_t out_step_h, out_step_w, out_off_h, out_off_w;
    /* parameters */
    const float* packed_weights;     /* from mr_conv_pack_weights_f32 (device copy)              */
    const float* bias;               /* out_channels floats or NULL                              */
    const float* residual;           /* same geometry as dst (incl. channel offset) or NULL      */
    int32_t activation;              /* MR_ACT_*                                                 */
    float act_p0, act_p1;
    /* schedule */
    int32_t cout_blocks_per_wg;      /* MB: 16-channel output blocks per workgroup, one of 1,2,3,4,6 */
    int32_t pixel_blocks_per_wave;   /* NB: 16-pixel row segments per wave, one of 1,2,4            */
    int32_t chunk_channels;          /* CK: input channels staged per LDS chunk: 8,16,32,64,128    */
    int32_t split_k;                 /* >= 1; > 1 needs `workspace`                               */
    float* workspace;                /* split_k * phases * batch * ceil16(out_channels) * out_h * out_w floats */
    /* optional output phases (the 4 parities of ConvTranspose2d(k=4,s=2), model/layers.py:389):
     * num_phases == 4 runs four filter sets in ONE launch; phase p uses phase_weights[p], its own
     * pad_top/pad_left and output offset, and the common kh/kw/stride/out_step.  num_phases <= 1: ignored. */
    int32_t num_phases;
    const float* phase_weights[4];
    int32_t phase_pad_top[4], phase_pad_left[4], phase_out_off_h[4], phase_out_off_w[4];
    /* schedule, continued: waves per workgroup, 4 (0 = default) or 8.  8 waves share one LDS tile of twice the
     * rows: same LDS and DMA traffic per output as 4 waves with 2x pixel_blocks_per_wave, but two waves per
     * SIMD from every workgroup, which hides the chunk-fill stalls.  8 needs the direct-read dwordx4 path
     * (in_mode DIRECT, no in_transform, src_w % 4 == 0); otherwise MR_ERR_UNSUPPORTED. */
    int32_t waves_per_wg;
    /* MR_COMPUTE_F32 (0, default): v_mfma_f32_16x16x4_f32, exact fp32 products - the path that meets the 1e-4 parity bar.
     * MR_COMPUTE_BF16: v_mfma_f32_16x16x16_bf16 - packed_weights / phase_weights from mr_conv_pack_weights_bf16, the
     * activations (still fp32 in memory) are rounded to bf16 (nearest even) as the B fragment is formed, fp32 accumulate:
     * the numerics of "bf16 weights and activations, fp32 accumulate" (BASELINE configs[4]).  chunk_channels in
     * {16, 32, 64, 128}; LDS-DMA staged inputs only (in_mode DIRECT / UPSAMPLE2, no in_transform).
     * MR_COMPUTE_BF16X3 (EXPERIMENTAL, not yet validated on hardware): fp32-class accuracy on the bf16 matrix cores - every
     * operand is split into hi = bf16(x) and lo = bf16(x - hi) (16 mantissa bits together) and a*b is evaluated as
     * a_hi*b_hi + a_hi*b_lo + a_lo*b_hi with fp32 accumulation (three v_mfma_f32_16x16x16_bf16 per 16 channels instead of
     * four v_mfma_f32_16x16x4_f32, which run at 1/16 of the rate).  Weights from mr_conv_pack_weights_bf16x3; the same
     * restrictions as MR_COMPUTE_BF16.  CPU emulation over the whole network: depth error 4e-6 (fp32 path 1.3e-6, bar 1e-4). */
    int32_t compute_dtype;
    /* per-phase filter sizes (num_phases == 4): phase p sweeps phase_kh[p] x phase_kw[p] taps of phase_weights[p] (packed with
     * that size); 0 = the common kh / kw, which must be the maximum over the phases (it sizes the input tile).  This is how
     * layers.Upconv (nearest x2 -> pad(0,1,0,1) -> conv2x2, model/layers.py:349-356) runs on the LOW-resolution input: output
     * parity (py, px) is a (1+py) x (1+px) convolution with the 2x2 filter's rows / columns summed where both fall on the same
     * input pixel - 9 instead of 16 multiply-adds per 2x2 output block. */
    int32_t phase_kh[4], phase_kw[4];
    /* schedule, continued: 1 = the waves of a workgroup split K instead of the pixels - all of them sweep the same
     * pixel_blocks_per_wave blocks of 16 pixels, each every waves_per_wg-th k-step of a chunk, and the partial sums are reduced
     * through LDS in a fixed order.  waves_per_wg times more workgroups for layers with few output pixels, without the workspace
     * round trip and the finishing launch of split_k (which must be 1 here; MR_COMPUTE_F32, LDS-DMA staged inputs only). */
    int32_t k_split_waves;
} mr_conv_desc;

/* number of floats of the packed weight image for a conv with the given source split and schedule
 * (cout_blocks_per_wg, chunk_channels must equal the values later put into mr_conv_desc) */
size_t mr_conv_packed_weight_floats(int32_t out_channels, const int32_t* src_channels, int32_t num_src,
                                    int32_t kh, int32_t kw, int32_t cout_blocks_per_wg, int32_t chunk_channels);

/*
 * Host-side repack of an (out_channels, sum(src_channels), kh, kw) fp32 weight (nn.Conv2d layout,
 * row-major) into the MFMA A-fragment stream the kernel consumes. `dst` is host memory of
 * mr_conv_packed_weight_floats() floats; upload it once per layer.
 */
int mr_conv_pack_weights_f32(const float* weight, int32_t out_channels, const int32_t* src_channels,
                             int32_t num_src, int32_t kh, int32_t kw, int32_t cout_blocks_per_wg,
                             int32_t chunk_channels, float* dst);

/* The same two functions for MR_COMPUTE_BF16 launches: sources padded to multiples of 16 channels, weights rounded to bf16
 * (nearest even), 4 bf16 per lane and k-step (layout in csrc/conv_layout.h).  `dst` is still sized in floats. */
size_t mr_conv_packed_weight_floats_bf16(int32_t out_channels, const int32_t* src_channels, int32_t num_src,
                                         int32_t kh, int32_t kw, int32_t cout_blocks_per_wg, int32_t chunk_channels);
int mr_conv_pack_weights_bf16(const float* weight, int32_t out_channels, const int32_t* src_channels,
                              int32_t num_src, int32_t kh, int32_t kw, int32_t cout_blocks_per_wg,
                              int32_t chunk_channels, float* dst);

/* ... and for MR_COMPUTE_BF16X3 launches: per lane and k-step 4 bf16 `hi` followed by 4 bf16 `lo` (16 bytes), weight image twice
 * the bf16 one (= the fp32 size for 16-aligned channel counts). */
size_t mr_conv_packed_weight_floats_bf16x3(int32_t out_channels, const int32_t* src_channels, int32_t num_src,
                                           int32_t kh, int32_t kw, int32_t cout_blocks_per_wg, int32_t chunk_channels);
int mr_conv_pack_weights_bf16x3(const float* weight, int32_t out_channels, const int32_t* src_channels,
                                int32_t num_src, int32_t kh, int32_t kw, int32_t cout_blocks_per_wg,
                                int32_t chunk_channels, float* dst);

/* bytes of dynamic LDS the launch will request (for planning / tests); negative MR_ERR_* if invalid */
int64_t mr_conv2d_lds_bytes(const mr_conv_desc* desc);

/* launch (replaces the reference lines listed above mr_conv_desc) */
int mr_conv2d_f32(const mr_conv_desc* desc, void* stream);

/*
 * 3x3, stride 1, zero padding 1 convolution (PadSameConv2d(3) + nn.Conv2d(3): every ConvReLU of the MaskModule,
 * model/monorec/monorec_model.py:296-343, model/layers.py:317-335; the 3x3 stride-1 convolutions of the ResNet trunk) as Winograd
 * F(2x2, 3x3) on the fp32 matrix cores: 16 multiplies per (input channel, output channel) and 2x2 output tile instead of 36.
 * Same conventions as mr_conv2d_f32: up to MR_MAX_SOURCES sources concatenated on channels and read in place, dense NCHW fp32,
 * bias / residual / activation (MR_ACT_NONE, MR_ACT_RELU, MR_ACT_LEAKY_RELU) in the epilogue, dst = (batch, out_channels, height,
 * width).  width % 4 == 0.  Results differ from the direct convolution by the rounding of the transforms (~1e-6 relative).
 */
typedef struct mr_wino_desc {
    const float* src[MR_MAX_SOURCES];
    int32_t src_channels[MR_MAX_SOURCES];
    int32_t num_src;
    int32_t batch, height, width;
    float* dst;
    int32_t out_channels;
    const float* packed_weights;     /* from mr_wino_pack_weights_f32 with the same cout_blocks_per_wave (device copy) */
    const float* bias;               /* out_channels floats or NULL */
    const float* residual;           /* same shape as dst or NULL */
    int32_t activation;
    float act_p0;
    int32_t cout_blocks_per_wave;    /* 1 or 2: a workgroup (8 waves, 8 x 32 output pixels) produces 32 or 64 output channels */
    int32_t variant;                 /* mr_conv3x3_winograd_f32 only: 0 input transform through an LDS buffer (thread = channel x tile),
                                        1 input transform in the registers of the lane that feeds it to the matrix core (no V buffer,
                                        one barrier per chunk; bit-identical results).  Which is faster is measured per layer shape.
                                        2 = 1 for out_channels = 32 a + r, 0 < r <= 16, cout_blocks_per_wave 1: the r tail channels are
                                        produced by workgroups of 16 x 32 pixels x 16 channels instead of a half-empty 32-channel group
                                        (the 48-channel layers); packed_weights then from mr_wino_pack_weights_tail_f32. */
    /* ---- mr_conv1d_cooktoom_f32 only (every other entry point wants them 0): strided source views and a column-split destination, which is
     * how the stride-2 halves of layers.ConvReLU2 (model/layers.py:289-314 with stride (2,1) / (1,2); monorec_model.py:489-501) run as stride-1
     * forms over [even samples | odd samples] (monorec_amd/cooktoom.py: stride2_as_stride1). */
    int32_t src_row_pitch;           /* floats between consecutive rows of a source as the launch sees it; 0 = width (dense).  2 * width with
                                        height = H / 2 reads every second row of an (.., H, width) tensor: src[s] = its first element for the even
                                        rows, + width floats for the odd rows */
    int32_t src_plane_floats;        /* floats between consecutive channel planes of a source in memory; 0 = height * width (dense) */
    int32_t dst_split_columns;       /* axis 1 only: 1 = the destination is stored de-interleaved by column parity, dst = (2, batch, out_channels,
                                        height, width / 2): [0] the even columns, [1] the odd ones - two dense tensors the 1 x k stride-(1,2) half
                                        of the pair reads as its two sources */
} mr_wino_desc;
size_t mr_wino_packed_weight_floats(int32_t out_channels, const int32_t* src_channels, int32_t num_src, int32_t cout_blocks_per_wave);
/* weight: (out_channels, sum(src_channels), 3, 3) fp32 host memory; the transformed filters G g G^T are formed in double */
int mr_wino_pack_weights_f32(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src,
                             int32_t cout_blocks_per_wave, float* dst);
/* variant 2: the full 32-channel groups as above (cout_blocks_per_wave 1), then the tail group of 1..16 channels */
size_t mr_wino_packed_weight_floats_tail(int32_t out_channels, const int32_t* src_channels, int32_t num_src);
int mr_wino_pack_weights_tail_f32(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src, float* dst);
int64_t mr_conv3x3_winograd_lds_bytes(const mr_wino_desc* desc);   /* dynamic LDS of the launch, or a negative MR_ERR_* code */
int mr_conv3x3_winograd_f32(const mr_wino_desc* desc, void* stream);

/*
 * The same 3x3 stride-1 convolution as Winograd F(4x4, 3x3): 36 multiplies per (input channel, output channel) and 4x4 outputs instead of
 * 144 (F(2x2, 3x3): 64) - the F(4, 3) Cook-Toom form of cooktoom_1d.h in both directions (points 0, +-1, +-2, infinity; transform
 * coefficients up to 8, transformed weights formed in double and rounded once).  Effect on the path's outputs measured before the kernel was
 * written (oracle/numerics_study_winograd.py: depth moves by 2.4e-7 with every 3x3 stride-1 layer of the mask and depth nets evaluated this
 * way).  Same descriptor and conventions as mr_conv3x3_winograd_f32 (`cout_blocks_per_wave` and `variant` ignored); a workgroup (8 waves)
 * produces 16 x 64 output pixels x 32 output channels and uses 153 KB of LDS, so it pays where the layer has >= 256 such workgroups.
 *
 * In the product library again since ABI 17 (ABI 16 had moved it to the diagnostic build: at c2 it buys nothing end to end); measured on
 * the c3 and configs[4] shapes it is 12-15 % ahead of the best F(2x2,3x3) variant on every full- and half-resolution 3x3 layer
 * (tools/sessions/r04_s18.sh), and only those table entries select it.
 */
size_t mr_wino44_packed_weight_floats(int32_t out_channels, const int32_t* src_channels, int32_t num_src);
int mr_wino44_pack_weights_f32(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src, float* dst);
int64_t mr_conv3x3_winograd44_lds_bytes(const mr_wino_desc* desc);
int mr_conv3x3_winograd44_f32(const mr_wino_desc* desc, void* stream);

/* The same F(4x4, 3x3) convolution with the 36 positions of a tile split over two waves (csrc/conv_wino44s.hip, round 5): a wave holds the 18
 * accumulator sets of one half of the vertical transform index and forms a partial output transform; the halves are added through LDS after the K
 * loop.  8 x 64 output pixels x 32 channels per workgroup, K in chunks of 4 channels, 70.5 KB of LDS and <= 128 registers: TWO workgroups per CU
 * (mr_conv3x3_winograd44_f32: one, whose load / transform / MFMA phases add up instead of overlapping).  Same products and transformed weights
 * as that kernel; the output differs by the rounding of a two-term partial sum.  Selected per layer shape by the measured table (code 41). */
size_t mr_wino44s_packed_weight_floats(int32_t out_channels, const int32_t* src_channels, int32_t num_src);
int mr_wino44s_pack_weights_f32(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src, float* dst);
int64_t mr_conv3x3_winograd44s_lds_bytes(const mr_wino_desc* desc);
int mr_conv3x3_winograd44s_f32(const mr_wino_desc* desc, void* stream);

/* The same F(4x4, 3x3) convolution with ONE WAVE PER SIMD (csrc/conv_wino44w.hip, round 6, ABI 19): 4 waves of 512 registers on 16 x 64 output pixels x 32
 * channels; a wave owns a tile row and BOTH 16-channel blocks (72 accumulator sets), so the input transform - VALU work that runs on the same ALUs as
 * the fp32 MFMAs - is done once per 72 MFMAs instead of once per 36, and the patch reads of the next channel quad are in flight while the current
 * quad multiplies; K in single-quad stages through a ring of four (partial vmcnt waits).  Packed weights of mr_wino44_pack_weights_f32; the same
 * products as mr_conv3x3_winograd44_f32, summed in the same order per output (bit-identical results).  Table code 51. */
int64_t mr_conv3x3_winograd44w_lds_bytes(const mr_wino_desc* desc);
int mr_conv3x3_winograd44w_f32(const mr_wino_desc* desc, void* stream);

/* Exported by the DIAGNOSTIC build only (python -m monorec_amd.build --timeline -> libmonorec_hip_timeline.so, selected with MR_HIP_LIBRARY):
 * bit 0 = the F(2,7) instantiations of mr_conv1d_cooktoom_f32 are present (no measured table entry ever selected them). */
#ifdef MR_DIAGNOSTIC_LIBRARY
int mr_diagnostic_forms(void);
#endif

/*
 * ---- bf16 MFMA path with channel-blocked bf16 activation storage (BASELINE configs[4]; MonoRecModel(hip_bf16=True)) --------------------
 * Layout "B8" of an activation: (batch, ceil(C / 8), H, W, 8) bf16 - one 16-byte group holds 8 consecutive channels of one pixel, padded
 * channels are zero.  mr_conv2d_b8 stands in for the nn.Conv2d / ConvTranspose2d(4,2) / Upconv layers of MaskModule and DepthModule
 * (model/monorec/monorec_model.py:345-385,526-557; model/layers.py:289-356,380-400): sources concatenated on channels and read in place,
 * each either B8 or dense fp32 NCHW (rounded to bf16, nearest even, while it is staged); v_mfma_f32_16x16x32_bf16 with fp32 accumulation;
 * bias and activation (none / ReLU / LeakyReLU(act_p0)) in the epilogue; destination B8 (rounded once) or fp32 NCHW, written at
 * (oy * out_step_h + phase_out_off_h, ox * out_step_w + phase_out_off_w) of a (dst_plane_h, dst_plane_w) plane.  Taps read input
 * (oy * stride_h - phase_pad_top + ky, ox * stride_w - phase_pad_left + kx), zero outside.  num_phases = 4 runs the four output parities of
 * a transposed / upsampling layer in one launch (per-phase filter size <= kh x kw, padding, offset, weights); num_phases <= 1 uses entry 0.
 * Not within the 1e-4 parity bar (bf16 operands): the accuracy bar of this mode is tests/test_gpu_model.py::test_c5_shape_in_fp32_and_bf16.
 */
#define MR_LAYOUT_F32_NCHW 0
#define MR_LAYOUT_BF16_B8  1
typedef struct mr_b8_conv_desc {
    const void* src[MR_MAX_SOURCES];
    int32_t src_channels[MR_MAX_SOURCES];
    int32_t src_layout[MR_MAX_SOURCES];      /* MR_LAYOUT_* */
    int32_t num_src, batch, src_h, src_w;
    int32_t kh, kw, stride_h, stride_w;      /* kh / kw: the maximum over the phases */
    int32_t out_h, out_w;                    /* conv grid size (per phase) */
    void* dst;
    int32_t dst_layout, out_channels;
    int32_t dst_plane_h, dst_plane_w, out_step_h, out_step_w;
    const float* bias;                       /* out_channels floats or NULL */
    int32_t activation;
    float act_p0;
    int32_t cout_blocks_per_wg;              /* MB: 1..4 blocks of 16 output channels per workgroup */
    int32_t pixel_blocks_per_wave;           /* NB: 1, 2, 4 */
    int32_t waves_per_wg;                    /* 4 or 8 */
    int32_t num_phases;
    const void* phase_weights[4];            /* from mr_b8_pack_weights with that phase's filter size (device copies) */
    int32_t phase_kh[4], phase_kw[4];        /* 0 = kh / kw */
    int32_t phase_pad_top[4], phase_pad_left[4], phase_out_off_h[4], phase_out_off_w[4];
} mr_b8_conv_desc;
size_t mr_b8_packed_weight_bytes(int32_t out_channels, const int32_t* src_channels, int32_t num_src, int32_t kh, int32_t kw, int32_t mb);
/* weight: (out_channels, sum(src_channels), kh, kw) fp32 in host memory -> bf16 A-fragment stream in host memory `dst` */
int mr_b8_pack_weights(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src, int32_t kh, int32_t kw,
                       int32_t mb, void* dst);
int64_t mr_conv2d_b8_lds_bytes(const mr_b8_conv_desc* desc);
int mr_conv2d_b8(const mr_b8_conv_desc* desc, void* stream);
/* nn.MaxPool2d(2) of the next MaskModule encoder stage and the maximum over the frames (monorec_model.py:357-365) on B8 tensors:
 * src (frames, planes, h, w) 16-byte groups, planes = batch * channel blocks -> pooled (frames, planes, h/2, w/2), fmax (planes, h, w) */
int mr_pool2x2_framemax_b8(const void* src, void* pooled, void* fmax, int32_t frames, int64_t planes, int32_t h, int32_t w, void* stream);
int mr_max_over_frames_b8(const void* src, void* dst, int32_t frames, int64_t groups16, void* stream);
/* The two producers of the nets' fp32 inputs, writing a B8 copy on the side so that the first layers read no fp32 volume:
 * mr_cost_volume_b8_f32 = mr_cost_volume_mode_f32 of the default configuration (3x3 patch, sfcv * mask; 32 / 48 / 64 depth steps) with
 * sfcv_b8[f] = (batch, num_depths / 8, height, width, 8) bf16 per frame next to the dense single-frame volumes (which stay the outputs).
 * Being the entry point of the bf16 configuration only (accuracy bar 1e-2 / 1e-3 on the depth), it forms the 3x3 window sums separably and
 * multiplies by fp32(1/9) where mr_cost_volume_f32 keeps the reference's summation order and division: -17 % instructions; the volumes differ
 * from mr_cost_volume_f32's by <= 1e-4 (the fused volume by more where the frame weights nearly cancel, as between any two summation orders),
 * validity (the zeros of the volumes) exactly equal;
 * mr_mask_classifier_b8_f32 = mr_mask_classifier_f32 with the masked volume (monorec_model.py:713) also as
 * cost_volume_b8 = (batch, num_depths / 8, plane, 8) bf16 (num_depths % 16 == 0). */
int mr_cost_volume_b8_f32(const float* keyframe, const float* const* frames, int32_t num_frames, const float* kinv, const float* proj,
                          const float* depths, int32_t batch, int32_t num_depths, int32_t height, int32_t width, float alpha,
                          const float* channel_weights, int32_t use_ssim, const float* pixel_depths, float* cost_volume,
                          float* const* sfcv, void* const* sfcv_b8, void* stream);
/* mr_cost_volume_b8_f32 for a caller that does not hand out fp32 single-frame volumes (MonoRecModel(hip_bf16=True, hip_lean_outputs=True)):
 * the fusion kernel writes the fused volume and the B8 copies only; sfcv[f] are SCRATCH (they end up holding the raw per-frame costs, not
 * monorec_model.py:251's volumes) - D * F * H * W * 4 bytes of HBM writes less per keyframe (403 MB at BASELINE configs[4]). */
int mr_cost_volume_b8_lean_f32(const float* keyframe, const float* const* frames, int32_t num_frames, const float* kinv, const float* proj,
                               const float* depths, int32_t batch, int32_t num_depths, int32_t height, int32_t width, float alpha,
                               const float* channel_weights, int32_t use_ssim, const float* pixel_depths, float* cost_volume,
                               float* const* sfcv_scratch, void* const* sfcv_b8, void* stream);
int mr_mask_classifier_b8_f32(const float* features, const float* weight, const float* bias, int32_t batch, int32_t channels, int64_t plane,
                              float* cv_mask, float* cost_volume, int32_t num_depths, void* cost_volume_b8, void* stream);
/* layout conversions: dense fp32 (n, c, hw) <-> B8 (n, ceil(c/8), hw, 8) bf16 */
int mr_f32_nchw_to_b8(const float* src, void* dst, int32_t n, int32_t c, int64_t hw, void* stream);
int mr_b8_to_f32_nchw(const void* src, float* dst, int32_t n, int32_t c, int64_t hw, void* stream);

/*
 * 3x1 / 1x3, stride 1, zero padding 1 along the filter axis (PadSameConv2d + nn.Conv2d of layers.ConvReLU2, model/layers.py:289-314: the
 * second pair of every DepthModule encoder stage, dec{1,2}.1, dec4.0 - model/monorec/monorec_model.py:485-513) as 1-D Winograd F(2, 3):
 * 4 multiplies per (input channel, output channel) and 2 outputs instead of 6.  Same descriptor and conventions as
 * mr_conv3x3_winograd_f32 (sources concatenated on channels and read in place, bias / activation in the epilogue, dst = (batch,
 * out_channels, height, width), width % 4 == 0); no residual; `variant` ignored; cout_blocks_per_wave 1..4: a workgroup (8 waves, 8 x 32
 * output pixels) produces 16 x that many output channels.  axis 0: 1 x 3 (along x), weight (out, in, 1, 3); axis 1: 3 x 1 (along y),
 * weight (out, in, 3, 1) - three taps per (out, in) in memory either way.
 */
size_t mr_wino1d_packed_weight_floats(int32_t out_channels, const int32_t* src_channels, int32_t num_src, int32_t cout_blocks_per_wave);
int mr_wino1d_pack_weights_f32(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src,
                               int32_t cout_blocks_per_wave, float* dst);
int64_t mr_conv1d3_winograd_lds_bytes(const mr_wino_desc* desc);
int mr_conv1d3_winograd_f32(const mr_wino_desc* desc, int32_t axis, void* stream);

/*
 * The larger Cook-Toom forms of the same layers: F(m, r) = m outputs along the filter axis from m + r - 1 inputs with m + r - 1
 * multiplies per (input channel, output channel).  (m, r) = (4, 3): 6 instead of 12 multiplies per 4 outputs of the 3-tap layers;
 * (2, 7) / (4, 7): 8 / 10 instead of 14 / 28 for the 7 x 1 and 1 x 7 stride-1 layers of DepthModule.enc.0.0
 * (model/monorec/monorec_model.py:487-500, layers.ConvReLU2 model/layers.py:289-314).  Interpolation points 0, +-1, +-2, +-1/2, +-4,
 * infinity; transform coefficients are dyadic rationals, the transformed weights are formed in double and rounded once.  Effect on the
 * path's outputs measured before the kernel was written (oracle/numerics_study_winograd.py: depth moves by <= 4e-7).  Descriptor and
 * conventions as mr_conv1d3_winograd_f32 (zero padding (r - 1) / 2 either side, width % 4 == 0, no residual); weight (out, in, 1, r) for
 * axis 0, (out, in, r, 1) for axis 1; cout_blocks_per_wave 1..4 (1..3 for (4, 7)).  A workgroup (8 waves) produces 8 rows x 16 m
 * columns (axis 0) or 4 m rows x 32 columns (axis 1).  MR_ERR_BAD_ARGUMENT for any other (m, r).
 */
size_t mr_cooktoom1d_packed_weight_floats(int32_t out_channels, const int32_t* src_channels, int32_t num_src, int32_t cout_blocks_per_wave,
                                          int32_t m, int32_t r);
int mr_cooktoom1d_pack_weights_f32(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src,
                                   int32_t cout_blocks_per_wave, int32_t m, int32_t r, float* dst);
int64_t mr_conv1d_cooktoom_lds_bytes(const mr_wino_desc* desc, int32_t axis, int32_t m, int32_t r);
int mr_conv1d_cooktoom_f32(const mr_wino_desc* desc, int32_t axis, int32_t m, int32_t r, void* stream);

/*
 * layers.Upconv (model/layers.py:349-356: nn.Upsample(2, nearest) -> pad (0,1,0,1) -> nn.Conv2d(2); the first layer of every MaskModule
 * decoder stage, model/monorec/monorec_model.py:318-338) with 4 multiplies per (input channel, output channel) and 2x2 output block
 * instead of 16 (9 as four parity phases of mr_conv2d_f32): the block of input position (y, x) is a bilinear form of the 2x2 input patch
 * at (y, x), evaluated on differences of neighbouring inputs.  Same descriptor as the functions above: sources (batch, C_s, height, width)
 * are the LOW-resolution input, dst = (batch, out_channels, 2 height, 2 width), bias / activation in the epilogue, no residual,
 * cout_blocks_per_wave 1 or 2 (16 or 32 output channels per workgroup), width % 4 == 0.
 */
int mr_upconv_pack_weights_f32(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src,
                               int32_t cout_blocks_per_wave, float* dst);      /* size: mr_wino1d_packed_weight_floats */
int mr_upconv2x2_winograd_f32(const mr_wino_desc* desc, void* stream);

/*
 * nn.ConvTranspose2d(kernel 4, stride 2) + the centre crop of layers.Refine (model/layers.py:380-400: the decoder stages of the
 * DepthModule, model/monorec/monorec_model.py:503-513) as Winograd F(2x2, 2x2): each of the four output parities is a 2x2 stride-1
 * convolution on the low-resolution input (9 multiplies per 2x2 parity tile instead of 16; transform coefficients 0 / +-1 only).
 * Same descriptor as mr_conv3x3_winograd_f32: sources (batch, C_s, height, width) read in place, dst = (batch, out_channels,
 * 2 * height, 2 * width), bias / activation in the epilogue, no residual; cout_blocks_per_wave 1, 2 or 4 (32 / 64 / 128 output channels
 * per workgroup); packed_weights from mr_wino_t_pack_weights_f32 with the same value.  width % 4 == 0.  `variant` as for
 * mr_conv3x3_winograd_f32 (0 transform through LDS, 1 in registers, 2 = 1 with 16-channel tail workgroups).
 */
size_t mr_wino_t_packed_weight_floats(int32_t out_channels, const int32_t* src_channels, int32_t num_src, int32_t cout_blocks_per_wave);
/* weight: the nn.ConvTranspose2d tensor (sum(src_channels), out_channels, 4, 4), fp32 host memory */
int mr_wino_t_pack_weights_f32(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src,
                               int32_t cout_blocks_per_wave, float* dst);
/* variant 2 (out_channels = 32 a + r, 0 < r <= 16, cout_blocks_per_wave 1): full 32-channel groups, then the tail group of r channels */
size_t mr_wino_t_packed_weight_floats_tail(int32_t out_channels, const int32_t* src_channels, int32_t num_src);
int mr_wino_t_pack_weights_tail_f32(const float* weight, int32_t out_channels, const int32_t* src_channels, int32_t num_src, float* dst);
int64_t mr_convt4x4s2_winograd_lds_bytes(const mr_wino_desc* desc);
int mr_convt4x4s2_winograd_f32(const mr_wino_desc* desc, void* stream);

/*
 * Fused plane-sweep cost volume.  Replaces CostVolumeModule.forward per-pixel work,
 * model/monorec/monorec_model.py:193-271 (+ model/layers.py:63-71 point_projection,
 * :119-137 SSIM, F.grid_sample x2, F.conv3d), for use_mono, use_ssim=True, sfcv_mult_mask=True,
 * patch_size=3.  The 4x4 pose/intrinsics algebra of :171,198,207 stays on the host:
 *   kinv   : batch x 9      inverse(keyframe_intrinsics)[:3,:3], row-major
 *   proj   : batch x F x 12 (K_f @ (inverse(pose_f) @ pose_kf))[:3,:4], row-major
 *   depths : D depth hypotheses (1/linspace(inv_max, inv_min, D)), far to near
 * keyframe: (batch,3,H,W); frames[f]: (batch,3,H,W), all in [-0.5,0.5].
 * Outputs: cost_volume (batch,D,H,W); sfcv[f] (batch,D,H,W).
 * D >= 2 (any parity: the kernels take the planes in pairs, an odd D's last pair repeats the last hypothesis and drops its second plane), F <= MR_MAX_FRAMES.  sfcv[f] doubles as scratch for the raw matching cost between the two
 * internal launches (sad kernel, per-pixel fusion kernel); no other workspace is needed.
 */
int mr_cost_volume_f32(const float* keyframe, const float* const* frames, int32_t num_frames,
                       const float* kinv, const float* proj, const float* depths,
                       int32_t batch, int32_t num_depths, int32_t height, int32_t width,
                       float alpha, const float* channel_weights /* 3 host floats */,
                       float* cost_volume, float* const* sfcv, void* stream);

/* The same with the photometric term selected like CostVolumeModule's use_ssim (monorec_model.py:227-243):
 * 1 = SSIM distance (what mr_cost_volume_f32 does), 0 = absolute difference, 2 = 0.85 SSIM + 0.15 absolute difference,
 * 3 = absolute difference averaged over 3x3 (zero padded); and, when pixel_depths != NULL, per-pixel depth hypotheses
 * (batch, num_depths, H, W) instead of the num_depths shared ones - data_dict["cv_depths"], monorec_model.py:181-182
 * (`depths` may then be NULL); and sfcv_mult_mask = 0 masks the single-frame volumes per depth plane by
 * (any channel of the warped pixel != 0) | (warped pixel == keyframe pixel) instead of by the all-depth validity
 * (monorec_model.py:252-253; needs num_depths >= num_frames), 1 = default. */
int mr_cost_volume_mode_f32(const float* keyframe, const float* const* frames, int32_t num_frames,
                            const float* kinv, const float* proj, const float* depths,
                            int32_t batch, int32_t num_depths, int32_t height, int32_t width,
                            float alpha, const float* channel_weights, int32_t use_ssim,
                            const float* pixel_depths, int32_t sfcv_mult_mask,
                            float* cost_volume, float* const* sfcv, void* stream);

/* Opt-in of the fp32 path (MonoRecModel(hip_cv_separable=True)): mr_cost_volume_mode_f32 of the default configuration (3x3 patch,
 * sfcv * mask) with the 3x3 window sums of layers.SSIM (model/layers.py:123-131) and of the box stage (monorec_model.py:246-248) formed
 * SEPARABLY (every row keeps its horizontal sums; a window is (top + mid) + cur) and x * fp32(1/9) for x / 9 - another rounding of the same
 * nine-term sums, -17 % instructions in the sad kernel.  Validity (the zeros of the volumes) is exactly mr_cost_volume_f32's; single-frame
 * volumes differ by <= 1e-4, the depth by <= 2e-6 (inside north_star's 1e-4-on-depth bar; the DEFAULT stays the exact-order kernel, whose
 * volumes agree with the reference to 5e-7).  Per-pixel depths / sizes without an exact constant division run the exact kernels. */
int mr_cost_volume_relaxed_f32(const float* keyframe, const float* const* frames, int32_t num_frames,
                               const float* kinv, const float* proj, const float* depths,
                               int32_t batch, int32_t num_depths, int32_t height, int32_t width,
                               float alpha, const float* channel_weights, int32_t use_ssim, const float* pixel_depths,
                               float* cost_volume, float* const* sfcv, void* stream);

/* mr_cost_volume_mode_f32 on the round-1 kernels (LDS-tiled sad kernel + three-pass fusion kernel) whatever the options: the
 * default configuration (use_ssim 1, sfcv_mult_mask 1) otherwise runs the LDS-free marching kernel + register-resident fusion
 * kernel, whose results are bit-identical.  Kept as the A/B reference of that claim (tests/test_gpu_kernels.py) and for timing. */
int mr_cost_volume_tiled_f32(const float* keyframe, const float* const* frames, int32_t num_frames,
                             const float* kinv, const float* proj, const float* depths,
                             int32_t batch, int32_t num_depths, int32_t height, int32_t width,
                             float alpha, const float* channel_weights, int32_t use_ssim,
                             const float* pixel_depths, int32_t sfcv_mult_mask,
                             float* cost_volume, float* const* sfcv, void* stream);

/* The same with a P x P matching patch, `cv_patch_size` of MonoRecModel (monorec_model.py:138-142,247): the photometric term is
 * averaged over a zero-padded patch_size x patch_size box and the border radius becomes patch_size / 2 + 1 (:139).
 * patch_size odd, 1..7; 3 is the tuned kernel of mr_cost_volume_mode_f32, the others run a generic (slower) variant. */
int mr_cost_volume_patch_f32(const float* keyframe, const float* const* frames, int32_t num_frames,
                             const float* kinv, const float* proj, const float* depths,
                             int32_t batch, int32_t num_depths, int32_t height, int32_t width,
                             float alpha, const float* channel_weights, int32_t use_ssim,
                             const float* pixel_depths, int32_t sfcv_mult_mask, int32_t patch_size,
                             float* cost_volume, float* const* sfcv, void* stream);

/* nn.MaxPool2d(kernel 3, stride 2, padding 1) of the torchvision ResNet stem (monorec_model.py:124) */
int mr_maxpool3x3s2_f32(const float* src, float* dst, int32_t planes, int32_t in_h, int32_t in_w, void* stream);

/* nn.MaxPool2d(2) between the MaskModule encoder stages (monorec_model.py:304-316). in_h even, in_w % 4 == 0.
 * (mr_conv2d_f32 can also pool while staging - MR_IN_MAXPOOL2 - but the separate pass + DMA-staged conv is
 * faster on MI355X.) */
int mr_maxpool2x2_f32(const float* src, float* dst, int64_t planes, int32_t in_h, int32_t in_w, void* stream);

/* MonoRecModel.forward returns tensors the caller owns (the reference's outputs are fresh tensors: monorec_model.py:256-279,
 * 690, 713-727; create_pointcloud.py:79-98 keeps `result` of five keyframes and multiplies one in place).  The path computes into
 * resident buffers, so forward() ends with ONE launch that copies every output into the caller's memory: `num_segments`
 * (<= MR_MAX_COPY_SEGMENTS) independent device-to-device copies; src / dst 16-byte aligned, bytes a positive multiple of 16. */
#define MR_MAX_COPY_SEGMENTS 24
typedef struct mr_copy_segment {
    const void* src;
    void* dst;
    int64_t bytes;
} mr_copy_segment;
int mr_copy_segments(const mr_copy_segment* segments, int32_t num_segments, void* stream);

/* Host helper of the cost-volume launch: 1 when the 3-instruction reciprocal sequence the kernels use for `u / (W - 1)`, `v / (H - 1)`
 * (model/layers.py:67-68) reproduces the correctly rounded fp32 quotient for every dividend (exhaustive over a binade, cached per
 * divisor), 0 when the launch must use IEEE division for this divisor.  Exposed so that tests can pin the verdicts. */
int mr_exact_const_division(float divisor);

/* Host query of the cost-volume launch decision: what the mr_cost_volume_* entry points launch for a set of arguments, filled by the very
 * function the launchers consume (one copy of the rules).  It never touches the device.  The arguments are those of the entry points the
 * decision depends on; pointers are taken as given (`has_pixel_depths`, `has_b8`: pixel_depths / sfcv_b8 non-null), `tiled` selects
 * mr_cost_volume_tiled_f32, `relaxed` mr_cost_volume_relaxed_f32, `lean` mr_cost_volume_b8_lean_f32 (with has_b8).  Returns out->status:
 * 0, or the MR_ERR_* code the entry point returns for these arguments (every other field is then 0); MR_ERR_BAD_ARGUMENT for out == NULL.
 * Exposed so that tests can pin which kernel instantiation a shape runs (tests/cost_volume_paths.py). */
enum { MR_CV_FAMILY_MARCH = 1, MR_CV_FAMILY_TILED = 2, MR_CV_FAMILY_PATCH = 3 };
enum { MR_CV_FUSE_REG = 1, MR_CV_FUSE_GENERIC = 2 };
typedef struct mr_cv_launch {
    int32_t status;
    int32_t family;                 /* MR_CV_FAMILY_*: cv_sad_march_kernel / cv_sad_kernel / cv_sad_patch_kernel */
    int32_t mode, opt;              /* MODE = use_ssim; OPT bit 0 per-pixel depths, bit 1 per-plane flags (sfcv_mult_mask = 0) */
    int32_t sad_grid[3], sad_block; /* grid and workgroup size of the sad kernel */
    /* marching kernel (family MARCH; 0 otherwise): template arguments, geometry, and whether cv_kf_stats_kernel runs first */
    int32_t dp, pixd, kfs, fd, relaxed;
    int32_t strips, pitch, ty, ysegs, npairs;
    int32_t kf_prepass, kf_grid[2];
    /* tiled / patch kernels (0 for MARCH) */
    int32_t tile_w, tile_h, tiles_x, tiles, nchunk, dchunk;
    int32_t radius;                 /* patch_size / 2 */
    int32_t lds_bytes;              /* per workgroup: static (tiled) or dynamic (patch) */
    int32_t flag_memset;            /* 1: the cost-volume buffer is set to all ones (validity words) before the sad kernel */
    /* fusion kernel */
    int32_t fuse;                   /* MR_CV_FUSE_REG: cv_fuse_reg_kernel<fuse_depths, fuse_b8>; MR_CV_FUSE_GENERIC: cv_fuse_kernel<fuse_pflag> */
    int32_t fuse_depths, fuse_b8, fuse_lean, fuse_pflag;
    int32_t fuse_grid[2];
} mr_cv_launch;
int mr_cost_volume_launch_query(int32_t num_frames, int32_t batch, int32_t num_depths, int32_t height, int32_t width,
                                int32_t use_ssim, int32_t has_pixel_depths, int32_t sfcv_mult_mask, int32_t patch_size,
                                int32_t tiled, int32_t has_b8, int32_t relaxed, int32_t lean, mr_cv_launch* out);

/* `num` (<= MR_MAX_GATHER) small fp32 tensors of `floats_each` elements each, anywhere in device memory, -> dst[num][floats_each],
 * one launch.  MonoRecModel uses it to bring the 4x4 pose / intrinsics matrices of a forward (monorec_model.py:160-171: they feed
 * torch.inverse / matmul, which this implementation runs with the reference's CPU operators) into device-writable pinned host memory. */
#define MR_MAX_GATHER (2 + 2 * MR_MAX_FRAMES)
int mr_gather_small_f32(const float* const* srcs, int32_t num, int32_t floats_each, float* dst, void* stream);

/* A run of consecutive convolution launches behind ONE host call: item i names an entry point above (MR_LAUNCH_*) and its descriptor
 * (mr_conv_desc for MR_LAUNCH_CONV2D, mr_wino_desc otherwise; `arg` = the axis of mr_conv1d3_winograd_f32, or
 * axis | m << 4 | r << 8 for MR_LAUNCH_COOKTOOM_1D = mr_conv1d_cooktoom_f32).  Launched in order on
 * `stream`; stops at the first failure, returns its code and - if `failed_index` is given - its position.  (No reference equivalent:
 * the reference issues one ATen call per layer from Python; this is the launch-overhead side of MonoRecModel.forward.) */
#define MR_LAUNCH_CONV2D  0
#define MR_LAUNCH_WINO3X3 1
#define MR_LAUNCH_WINO_T  2
#define MR_LAUNCH_WINO_1D 3
#define MR_LAUNCH_UPCONV  4
#define MR_LAUNCH_COOKTOOM_1D 5
#define MR_LAUNCH_WINO44  6
#define MR_LAUNCH_CONV_B8 7
#define MR_LAUNCH_WINO44S 8
#define MR_LAUNCH_WINO44W 9
typedef struct mr_launch_item {
    int32_t kind;
    int32_t arg;
    const void* desc;
} mr_launch_item;
int mr_run_launches(const mr_launch_item* items, int32_t num, void* stream, int32_t* failed_index);

/* ResnetEncoder input normalisation ((x + 0.5) - 0.45) / 0.225, elementwise (monorec_model.py:691 + :120);
 * count % 4 == 0.  (MR_TF_RESNET_NORM does the same while staging inside mr_conv2d_f32.) */
int mr_resnet_normalize_f32(const float* src, float* dst, int64_t count, void* stream);

/* elementwise max over F stacked tensors: torch.max(cv_feats[i], x) (monorec_model.py:365).
 * src is (F, count) contiguous. */
int mr_max_over_frames_f32(const float* src, float* dst, int32_t num_frames, int64_t count, void* stream);

/* SimpleMaskModule input (monorec_model.py:448-449): stacked.sum(0) / (stacked != 0).sum(0).clamp_min(1) over the F
 * single-frame cost volumes.  src is (F, count) contiguous, count % 4 == 0. */
int mr_nonzero_mean_over_frames_f32(const float* src, float* dst, int32_t num_frames, int64_t count, void* stream);

/* Both consumers of a MaskModule encoder stage output in one pass: pooled = MaxPool2d(2) per frame (next stage input,
 * monorec_model.py:304-316) and frame_max = max over the frames (cv_feats[i], :365).
 * src (F, planes, in_h, in_w) -> pooled (F, planes, in_h/2, in_w/2), frame_max (planes, in_h, in_w);
 * planes = batch * channels, in_h even, in_w % 4 == 0. */
int mr_pool2x2_framemax_f32(const float* src, float* pooled, float* frame_max, int32_t num_frames, int64_t planes,
                            int32_t in_h, int32_t in_w, void* stream);

/* cost_volume = (1 - cv_mask) * cost_volume (monorec_model.py:713); mask (batch,1,H,W), cv (batch,D,H,W).
 * dst may alias cv. */
int mr_apply_mask_f32(const float* cv, const float* mask, float* dst, int32_t batch, int32_t num_depths,
                      int64_t plane, void* stream);

/* MaskModule.classifier = nn.Conv2d(C, 1, kernel_size=1) + nn.Sigmoid (monorec_model.py:340-343, applied :383) fused with the
 * mask multiply that follows it in MonoRecModel.forward, cost_volume = (1 - cv_mask) * cost_volume (:713):
 *   cv_mask[b,0,p] = sigmoid(bias[0] + sum_c weight[c] * features[b,c,p]);   cost_volume[b,d,p] *= 1 - cv_mask[b,0,p]  (in place)
 * features (batch, channels, plane) with plane = H*W even, weight (channels) = the conv's (1,C,1,1) tensor, cv_mask (batch,1,plane),
 * cost_volume (batch, num_depths, plane) or NULL (mask only: pretrain_mode 2, :712,723).  One HBM-bound launch instead of a
 * 1-of-16-rows MFMA launch + mr_apply_mask_f32. */
int mr_mask_classifier_f32(const float* features, const float* weight, const float* bias, int32_t batch, int32_t channels,
                           int64_t plane, float* cv_mask, float* cost_volume, int32_t num_depths, void* stream);

/* DepthModule.predictors[i] = PadSameConv2d(3) + nn.Conv2d(C_i, 1, 3) (monorec_model.py:520-523), predict_depth's abs(tanh(x))
 * (:554-557) and the inverse-depth affine (1 - p) * act_p0 + p * act_p1 of MonoRecModel.forward (:716-717), for up to
 * MR_MAX_HEADS heads in ONE launch (their inputs differ in size; nothing downstream reads the outputs, so they run together once
 * the decoder is done).  Per head: src (batch, channels, height, width), weight (1, channels, 3, 3) as nn.Conv2d stores it,
 * bias (1), dst (batch, 1, height, width); zero padding 1 on every side (PadSameConv2d of k=3, s=1: model/layers.py:249-251). */
typedef struct mr_head_desc {
    const float* src;
    const float* weight;
    const float* bias;
    float* dst;
    int32_t batch, channels, height, width;
} mr_head_desc;
int mr_depth_heads_f32(const mr_head_desc* heads, int32_t num_heads, float act_p0, float act_p1, void* stream);

/* Fused sparse depth metrics, one launch for all seven metrics of configs/evaluate/eval_monorec.json:53-61
 * (model/metric_functions/sparse_metrics.py:136-252 with utils/util.py:36-118; pred_all_valid=True, no cv-mask):
 * prediction/target (batch,1,H,W) inverse depths; roi = {y0,y1,x0,x1} host ints or NULL; max_distance <= 0 = None.
 * sums: batch x 8 doubles on the device, per sample [n_valid, sum|dp-dg|/dg, sum(dp-dg)^2/dg, sum(dp-dg)^2,
 * sum(log dp - log dg)^2, n(thresh<1.25), n(thresh<1.25^2), n(thresh<1.25^3)].
 * relu / clamp_min / max keep NaN like torch (as in mr_metric_stage_sums_f32): a NaN prediction or target at an unmasked pixel makes
 * the four error sums of its sample NaN and counts for none of the three thresholds - it is not scored as a depth of max_distance. */
int mr_sparse_metric_sums_f32(const float* prediction, const float* target, int32_t batch, int32_t height,
                              int32_t width, const int32_t* roi, float max_distance, double* sums, void* stream);

/* ---- median scaling and the dense-target metrics (evaluater/evaluater.py:36-43, utils/util.py:135-142,
 *      model/metric_functions/sparse_metrics.py:6-78) ------------------------------------------------------------
 *
 * Per-sample exact masked order statistics, mask = target > 0 over the whole (uncropped) image, one entry per sample:
 *   count          selection size
 *   target_median  lower median sorted[(count-1)/2] of target[mask] (torch.median); NaN when count == 0
 *   lo, hi         prediction[mask] sorted[(count-1)/2] and sorted[count/2]; NaN when count == 0
 *   nans, zeros, infs  number of NaN, +-0 and +-inf values in prediction[mask] (after mr_median_stage_scales_f32: non-zero
 *                  = present).  The values are only defined when nans == 0. */
typedef struct {
    int32_t count;
    float target_median;
    float lo, hi;
    int32_t nans, zeros, infs;
    int32_t reserved;
} mr_median_stats;

/* Bytes of device workspace mr_median_select_f32 needs: the compacted selections (2 x batch x height x width x 4). */
int64_t mr_median_select_workspace_bytes(int32_t batch, int32_t height, int32_t width);

/* Radix select over order-preserving keys of the fp32 bit patterns, integer LDS histograms: exact and deterministic.
 * prediction/target (batch,1,H,W); stats: batch entries on the device.  One workgroup per (sample, tensor). */
int mr_median_select_f32(const float* prediction, const float* target, int32_t batch, int32_t height, int32_t width,
                         void* workspace, mr_median_stats* stats, void* stream);

/* The reference's median_scaling applied num_stages times in a row (once per configured metric, evaluater.py:40-43):
 * scales[b * num_stages + j] = median(target) / median(prediction after stages 0..j-1) in fp32, each stage multiplying
 * the prediction by its ratio.  Derived from the stats by the exact recurrence (a positive ratio keeps the order of the
 * selection, a negative one reverses it; a 0 / inf ratio meeting an inf / 0 makes the selection NaN).  stats_out (may be
 * NULL or alias stats) receives the statistics after the last stage.  One wave, no host synchronisation. */
int mr_median_stage_scales_f32(const mr_median_stats* stats, int32_t batch, int32_t num_stages, float* scales,
                               mr_median_stats* stats_out, void* stream);

#define MR_MAX_METRIC_STAGES 16
#define MR_METRIC_DENSE 0x100   /* or-ed into a stage column: the dense-target form (no mask, sparse_metrics.py:6-78) */

/* One pass over prediction and target for up to MR_MAX_METRIC_STAGES metric evaluations.  Stage j multiplies the
 * prediction by scales[b * num_stages + j] (fp32, after the multiplies of stages 0..j-1; scales NULL = no scaling) and
 * feeds the sum of column stage_columns[j] & 0xff (1..7, the layout of mr_sparse_metric_sums_f32), masked like that
 * entry point or, with MR_METRIC_DENSE, over every pixel of the roi.  relu / clamp_min keep NaN like torch.
 * sums: batch x (2 + num_stages) doubles on the device: [#valid (sparse mask), #pixels of the roi, stage 0, ...]. */
int mr_metric_stage_sums_f32(const float* prediction, const float* target, int32_t batch, int32_t height, int32_t width,
                             const int32_t* roi, float max_distance, const float* scales, int32_t num_stages,
                             const int32_t* stage_columns, double* sums, void* stream);

/* ---- point-cloud path: create_pointcloud.py + utils/ply_utils.py -------------------------------
 *
 * Static-scene mask of one keyframe, create_pointcloud.py:76-77:
 *   mask = (cv_mask >= threshold); out = (F.conv2d(mask, ones(mask_fill+1, mask_fill+1), padding=mask_fill//2) < 1)
 * i.e. 1 where no moving pixel lies within +-mask_fill/2 (zero padding), else 0.  cv_mask, out: (batch,1,H,W);
 * mask_fill even (reference: 32, threshold .1). */
int mr_static_mask_f32(const float* cv_mask, float* out, int32_t batch, int32_t height, int32_t width,
                       float threshold, int32_t mask_fill, void* stream);

/* One PLYSaver.add_depthmap (utils/ply_utils.py:34-53) preceded by the mask vote of create_pointcloud.py:90-92:
 *   vote   = (sum_k static_masks[k]) > vote_above            (num_masks = 0: no masking; reference: 5 masks, > 4)
 *   depth  = 1 / (inv_depth * vote);  keep = min_d <= depth <= max_d, inside roi (y0,y1,x0,x1; python slice
 *            semantics; NULL = whole image), and uniform > dropout when `uniform` (the torch.rand_like of :45) is given
 *   point  = pose @ [depth * (kinv @ (x, y, 1)); 1]           (model/layers.py:56-61, ply_utils.py:47-49)
 *   colour = (image + .5) * 255
 * Kept points are appended in the reference's order (batch, then pixel row-major) as 6 floats x y z r g b to
 * `records` starting at record *cursor; *cursor (device memory) is advanced by the number of kept points even
 * beyond `capacity_records` (nothing is written past the capacity - the caller checks).  No host synchronisation.
 * inv_depth/uniform (batch,1,H,W), image (batch,3,H,W), kinv batch x 9 (inverse(intrinsics)[:3,:3]), pose batch x 16. */
int mr_pointcloud_append_f32(const float* inv_depth, const float* const* static_masks, int32_t num_masks,
                             float vote_above, const float* image, const float* kinv, const float* pose,
                             const float* uniform, float dropout, float min_d, float max_d, const int32_t* roi,
                             int32_t batch, int32_t height, int32_t width, float* records, int64_t capacity_records,
                             int64_t* cursor, void* stream);

/* ---- TSDF-fusion export (ABI 23; monorec_amd/tsdf_export.py): utils/util.py:78-92, save_frame_for_tsdf, up to its Image.fromarray ----
 *
 * One launch for a batch of keyframes, optionally preceded by the mask vote of create_pointcloud.py:90-92 (as in
 * mr_pointcloud_append_f32: vote = sum_k static_masks[k] > vote_above, inv_depth *= vote; num_masks = 0: no masking):
 *   depth  = int16(trunc(fp32(fp32(1 / inv_depth) * 100)))  - the low half of the truncating 32-bit conversion, as torch on x86 -,
 *            then 0 where negative (327.68 m and beyond wraps, |v| >= 2^31 and NaN give 0, so does inv_depth == 0),
 *            then 0 where fp32(depth) < min_cm and where fp32(depth) > max_cm  (centimetres; -INFINITY / +INFINITY: no threshold,
 *            NaN: MR_ERR_BAD_ARGUMENT)
 *   colour = uint8(trunc(fp32(fp32(keyframe + .5) * 255))), pixel-interleaved r g b
 * both restricted to crop = (y0, y1, x0, x1), the reference's order, 0 <= y0 < y1 <= height, 0 <= x0 < x1 <= width (NULL: whole image).
 * inv_depth (batch,1,H,W), keyframe (batch,3,H,W) in [-.5, .5]; depth (batch, y1-y0, x1-x0) int16, 8-byte aligned; colour
 * (batch, y1-y0, x1-x0, 3) bytes, 4-byte aligned.  Null pointers, sizes < 1, a crop outside the image or empty, num_masks >
 * MR_MAX_VOTE_MASKS: MR_ERR_BAD_ARGUMENT, nothing is launched. */
int mr_tsdf_frame_f32(const float* inv_depth, const float* keyframe, const float* const* static_masks, int32_t num_masks,
                      float vote_above, const int32_t* crop, float min_cm, float max_cm, int32_t batch, int32_t height,
                      int32_t width, int16_t* depth, uint8_t* colour, void* stream);

/* ---- Cross-view depth consistency (an addition inside ABI 24, symbols only; monorec_amd/consistency.py): a keyframe's inverse depth
 * checked against the inverse depth of neighbouring keyframes before it goes into a point cloud, an export or a volume.  No reference
 * lines stand behind it: the arithmetic below is the definition. */

/* One neighbouring keyframe of mr_depth_consistency_f32, passed by value in the launch arguments. */
typedef struct mr_consistency_view {
    float m[12];                 /* neighbour camera <- reference camera, 3 x 4 row-major (formed on the host in double, rounded once) */
    float back[12];              /* reference camera <- neighbour camera: the inverse of m, likewise */
    float fx, fy, cx, cy;        /* pixel intrinsics of the neighbour */
    const float* inv_depth;      /* height x width, device memory: the neighbour's inverse depth (the model's `result`), unfiltered */
} mr_consistency_view;

/* Filter inv_depth (height x width, intrinsics fx fy cx cy) against views[0 .. num_views) (HOST array, 1 <= num_views <=
 * MR_CONSISTENCY_MAX_VIEWS, all height x width).  All fp32, every operation rounded on its own, in this order; roundf rounds halves away
 * from zero.  A depth value `inv` is VALID iff inv > 0 and d = 1 / inv is finite and > 0 (NaN, 0, negative values, +inf and values whose
 * reciprocal overflows are not).  For reference pixel (x, y) with inv = inv_depth[y][x], d = 1 / inv:
 *   invalid: hits = 0, out = 0.  Otherwise
 *   X = ((x - cx) / fx) * d,  Y = ((y - cy) / fy) * d,  Z = d;  sum = d, n = 0;  for view j = 0 .. num_views - 1 in this order
 *   (the first failing step ends that view):
 *     1  q_r = ((m[4r] * X + m[4r+1] * Y) + m[4r+2] * Z) + m[4r+3]                                      require q_2 > 0
 *     2  u = roundf(fx_j * (q_0 / q_2) + cx_j),  v = roundf(fy_j * (q_1 / q_2) + cy_j)                  require 0 <= u < width, 0 <= v < height
 *     3  invn = views[j].inv_depth[v][u],  dn = 1 / invn  (nearest pixel, as mr_tsdf_integrate_f32)     require invn VALID
 *     4                                                                                                 require fabsf(dn - q_2) <= rel_tol * q_2
 *     5  Xn = ((u - cx_j) / fx_j) * dn,  Yn = ((v - cy_j) / fy_j) * dn,  Zn = dn;  p_r from `back` like q_r from m      require p_2 > 0
 *        unless max_reproj_px is +INFINITY:  ex = (fx * (p_0 / p_2) + cx) - x,  ey = (fy * (p_1 / p_2) + cy) - y
 *                                                                                    require ex * ex + ey * ey <= max_reproj_px * max_reproj_px
 *     6  n += 1,  sum = sum + p_2
 *   hits[y][x] = n;  out[y][x] = n < min_views ? 0 : average ? 1 / (sum / (float)(1 + n)) : inv
 * out (fp32) or hits (bytes) may be NULL, not both; out must not alias an input (the views hold unfiltered depth).  One asynchronous launch
 * on `stream`, no allocation, no synchronisation.  Null inv_depth or views, both outputs NULL, num_views outside 1 .. MR_CONSISTENCY_MAX_VIEWS,
 * a view without inv_depth, height / width < 1, height * width >= 2^31, NaN or negative rel_tol or max_reproj_px, min_views < 0:
 * MR_ERR_BAD_ARGUMENT, nothing is launched. */
int mr_depth_consistency_f32(const float* inv_depth, float fx, float fy, float cx, float cy, const mr_consistency_view* views,
                             int32_t num_views, float rel_tol, float max_reproj_px, int32_t min_views, int32_t average,
                             int32_t height, int32_t width, float* out, uint8_t* hits, void* stream);

/* ---- TSDF fusion (ABI 24; monorec_amd/tsdf_fusion.py): a dense voxel volume in device memory, the packed keyframes of mr_tsdf_frame_f32
 * integrated into it, the zero-crossing surface points out.  No reference lines stand behind these: the arithmetic below is the definition.
 *
 * The volume has nx x ny x nz voxels, x fastest (idx = (z * ny + y) * nx + x, a 64-bit index): tsdf fp32 (initially 1), weight fp32
 * (initially 0) and, optionally (colour NULL: none), 4 bytes r g b 0 per voxel (initially 0).  Voxel (x, y, z) lies at
 * p_a = origin_a + (float)i_a * voxel_size.  `origin`: 3 floats in HOST memory, read during the call.  tsdf / weight need 4-byte,
 * colour 4-byte alignment; rows that start on a 16-byte boundary are moved with 16-byte accesses.
 * Null required pointers, nx / ny / nz < 1, nx * ny * nz >= 2^40, voxel_size <= 0 (or NaN): MR_ERR_BAD_ARGUMENT, nothing is launched. */
int mr_tsdf_volume_reset_f32(float* tsdf, float* weight, uint8_t* colour, int32_t nx, int32_t ny, int32_t nz, void* stream);

/* One keyframe of mr_tsdf_integrate_f32, passed by value in the launch arguments. */
typedef struct mr_tsdf_view {
    float m[12];                 /* world -> camera, 3 x 4 row-major (the fp32 inverse of the camera -> world pose, inverted on the host) */
    float fx, fy, cx, cy;        /* pixel intrinsics of the packed image (after the crop) */
    const int16_t* depth_cm;     /* height x width, device memory: depth of mr_tsdf_frame_f32 (centimetres, 0 = no depth) */
    const uint8_t* colour;       /* height x width x 3, device memory; may be NULL when the volume has no colour */
} mr_tsdf_view;

/* Integrate frames[0 .. num_frames) (HOST array, 1 <= num_frames <= MR_TSDF_MAX_FRAMES), all height x width, into the volume in the order
 * given.  Every voxel is loaded once, updated by the frames in turn and stored once, and only if a frame updated it: the result equals
 * num_frames launches of one frame bit for bit.  All fp32, every operation rounded on its own, for voxel (x, y, z) and one frame:
 *   p_a   = origin_a + (float)i_a * voxel_size
 *   cam_r = ((m[4r] * p_x + m[4r+1] * p_y) + m[4r+2] * p_z) + m[4r+3]                       skip if cam_2 <= 0
 *   u = roundf(fx * (cam_0 / cam_2) + cx), v = roundf(fy * (cam_1 / cam_2) + cy)             skip unless 0 <= u < width, 0 <= v < height
 *   d = (float)depth_cm[v][u] / 100                                                          skip if d <= 0 or d > max_depth_m (+INFINITY: no limit)
 *   diff = d - cam_2                                                                         skip if diff <= -trunc
 *   dist = fminf(1, diff / trunc);  w_new = w_old + 1;  tsdf = (tsdf * w_old + dist) / w_new
 *   colour_c = (uint8)fminf(255, floorf(((float)colour_c * w_old + (float)pixel_c) / w_new + .5))     c = r, g, b
 *   weight = w_new
 * A workgroup owns MR_TSDF_TILE_X x _Y x _Z voxels and skips a frame when the tile's bounding sphere lies outside one of the frame's near
 * and four side planes (prepared here in double, pushed outwards by more than the half pixel of roundf and the fp32 evaluation can
 * move a voxel; a frame with fx <= 0 or fy <= 0 is never culled): no voxel of such a tile could have passed the cam_2 and image-bounds
 * tests, so culling changes no result; a tile every frame skips touches no memory.
 * Besides the cases above: frames NULL, num_frames outside 1 .. MR_TSDF_MAX_FRAMES, a frame without depth_cm, a colour volume with a frame
 * without colour, height / width < 1, trunc <= 0, NaN max_depth_m: MR_ERR_BAD_ARGUMENT. */
int mr_tsdf_integrate_f32(float* tsdf, float* weight, uint8_t* colour, int32_t nx, int32_t ny, int32_t nz, const float* origin,
                          float voxel_size, float trunc, float max_depth_m, const mr_tsdf_view* frames, int32_t num_frames,
                          int32_t height, int32_t width, void* stream);

/* Surface points at the edge crossings of the grid: for every voxel v and axis a whose neighbour n = v + e_a is inside the volume,
 * when weight[v] > min_weight, weight[n] > min_weight and (tsdf[v] < 0) != (tsdf[n] < 0):
 *   s = tsdf[v] / (tsdf[v] - tsdf[n]);  pos_a = (origin_a + (float)i_a * voxel_size) + s * voxel_size, the other two coordinates p of v
 *   value_c = floorf((float)C_v + s * ((float)C_n - (float)C_v) + .5)                       (0 without a colour volume)
 * One record of 6 floats x y z red green blue per point, the record of mr_pointcloud_append_f32, in no particular order.  A workgroup
 * owns a tile of MR_TSDF_TILE_X x _Y x _Z voxels (the vertex kernel of the mesh below, over the three axis edges of a voxel alone); it
 * draws its range of records with one atomicAdd on *cursor (int64 in device memory, set by the caller, normally to 0) and writes those
 * below capacity_records; *cursor ends advanced by the number of points whatever the capacity.  A tile with no seen negative voxel
 * in reach (its own voxels and one beyond its high faces) touches neither the records nor the cursor.  records NULL: count only
 * (capacity_records is ignored) - count, allocate exactly, zero the cursor, fill.  Voxel indices are 64 bit: volumes of 2^31 voxels
 * and more are served.  The launch has one workgroup per tile, so 2^31 tiles or more (it was: 2^31 blocks of 256 voxels) are
 * MR_ERR_BAD_ARGUMENT, as for mr_tsdf_integrate_f32, and so is - here and for the two mesh entries - nx > 2^31 - 35, ny > 2^31 - 11
 * or nz > 2^31 - 7, where the halo staged with the last tile would leave the int32 range.  cursor NULL, capacity_records < 0, NaN min_weight: MR_ERR_BAD_ARGUMENT. */
int mr_tsdf_extract_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny, int32_t nz,
                        const float* origin, float voxel_size, float min_weight, float* records, int64_t capacity_records,
                        int64_t* cursor, void* stream);

/* The same surface as a welded, indexed triangle mesh (two entries added within ABI 24: the change only adds symbols): marching
 * tetrahedra over the Kuhn split of every cube of eight voxels.  It has no ambiguous cases, so the mesh is a closed 2-manifold wherever
 * the voxels are seen; the price is about twice the triangles of marching cubes.
 *
 * Edges.  Voxel v = (x, y, z) owns seven edges (v, e) from v to v + d_e:
 *   d_0 = (1,0,0)  d_1 = (0,1,0)  d_2 = (0,0,1)  d_3 = (1,1,0)  d_4 = (1,0,1)  d_5 = (0,1,1)  d_6 = (1,1,1)
 * Edge (v, e) is ACTIVE when n = v + d_e is inside the volume, weight[v] > min_weight, weight[n] > min_weight and
 * (tsdf[v] < 0) != (tsdf[n] < 0); a tsdf of exactly 0 counts as outside.  The 7-bit mask of v has bit e set for every active (v, e).
 * Every active edge carries one vertex, all fp32, every operation rounded on its own:
 *   s = tsdf[v] / (tsdf[v] - tsdf[n]);  step = s * voxel_size;  p_k = origin_k + (float)i_k * voxel_size
 *   pos_k = p_k + step where d_e[k] = 1, p_k elsewhere
 *   value_c = floorf((float)C_v + s * ((float)C_n - (float)C_v) + .5)                       (0 without a colour volume)
 * as one record x y z red green blue; for e < 3 it equals the record of mr_tsdf_extract_f32 bit for bit.  Vertices whose positions
 * coincide (a tsdf of exactly 0) stay distinct.
 *
 * Tetrahedra.  The cube at c0 = v, all eight corners inside the volume, is split along its diagonal into one tetrahedron per
 * permutation (a, b, c) of the axes, with the corners c0, c1 = c0 + e_a, c2 = c1 + e_b, c3 = c2 + e_c = c0 + (1,1,1), in the order
 *   even: (x,y,z) (y,z,x) (z,x,y)     odd: (x,z,y) (z,y,x) (y,x,z)
 * Its six edges, each owned by its first corner: E01 = (c0, a), E12 = (c1, b), E23 = (c2, c), E02 = (c0, a + b), E13 = (c1, b + c),
 * E03 = (c0, d_6), where p + q is the diagonal type of the axis pair: x + y = 3, x + z = 4, y + z = 5.  A tetrahedron emits triangles only
 * when all four corners have weight > min_weight; then every edge between an inside (tsdf < 0) and an outside corner is active, and
 * with case = sum of 1 << i over the inside corners c_i an EVEN tetrahedron emits
 *    1  c0            (E01 E02 E03)                     14  c1 c2 c3      (E01 E03 E02)
 *    2  c1            (E01 E13 E12)                     13  c0 c2 c3      (E01 E12 E13)
 *    4  c2            (E02 E12 E23)                     11  c0 c1 c3      (E02 E23 E12)
 *    8  c3            (E03 E23 E13)                      7  c0 c1 c2      (E03 E13 E23)
 *    3  c0 c1         (E12 E02 E03) (E12 E03 E13)       12  c2 c3         (E12 E13 E03) (E12 E03 E02)
 *    5  c0 c2         (E01 E12 E23) (E01 E23 E03)       10  c1 c3         (E01 E03 E23) (E01 E23 E12)
 *    6  c1 c2         (E01 E13 E23) (E01 E23 E02)        9  c0 c3         (E01 E02 E23) (E01 E23 E13)
 *    0, 15            nothing
 * (two inside corners cut a quad: it is split along the diagonal from the first vertex listed).  An ODD tetrahedron - its chain
 * c1 - c0, c2 - c0, c3 - c0 is left-handed - swaps the last two vertices of every triangle.  So for a triangle (a, b, c) the normal
 * (b - a) x (c - a) points from the inside (tsdf < 0) to the outside, towards the camera that saw the surface.  Triangles of zero area
 * are kept: the topology does not depend on the values.
 *
 * mr_tsdf_mesh_vertices_f32: one record per active edge into `vertices`, in no particular order, and into vertex_base[idx(v)] (int32,
 * nx * ny * nz elements, caller-owned) the index of the first vertex of every voxel v that owns one; elements of voxels without an
 * active edge are left untouched.  The vertices of one voxel are consecutive in the order of e:
 *   index(v, e) = vertex_base[idx(v)] + popcount(mask(v) & ((1 << e) - 1))
 * mr_tsdf_mesh_triangles_f32: three int32 vertex indices per triangle into `triangles`, in no particular order; it recomputes the masks
 * from tsdf / weight / min_weight - which must be those of the vertex call - and reads vertex_base of the owners.
 * Cursor and capacity as in mr_tsdf_extract_f32: one atomicAdd per workgroup on *cursor (int64, device memory, set by the caller),
 * records at or beyond the capacity are counted and not written.  vertices / triangles NULL: count only (capacity and vertex_base are
 * ignored; vertex_base may be NULL).  Indices are int32: a caller whose vertex count reaches 2^31 must not fill.  A workgroup owns
 * MR_TSDF_TILE_X x _Y x _Z voxels; a tile with no seen negative voxel in reach touches neither vertex_base nor the cursor.
 * Besides the cases of mr_tsdf_extract_f32: nx * ny * nz >= 2^31, vertex_base / triangles off a 4-byte boundary, an output without
 * vertex_base, a negative capacity with an output: MR_ERR_BAD_ARGUMENT, nothing is launched. */
int mr_tsdf_mesh_vertices_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny, int32_t nz,
                              const float* origin, float voxel_size, float min_weight, float* vertices, int64_t capacity_vertices,
                              int32_t* vertex_base, int64_t* cursor, void* stream);
int mr_tsdf_mesh_triangles_f32(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float min_weight,
                               const int32_t* vertex_base, int32_t* triangles, int64_t capacity_triangles, int64_t* cursor,
                               void* stream);

/* The volume seen from a camera (two entries added within ABI 24: the change only adds symbols): every pixel's ray is marched through
 * the volume in steps of `step` metres of camera z - the depth mr_tsdf_integrate_f32 fuses - until the trilinear tsdf turns from
 * non-negative to negative between two valid samples; the crossing's depth, the surface normal and the colour there come out.
 *
 * mr_tsdf_skip_grid_u8: one byte per brick of MR_TSDF_BRICK^3 voxels, ceil(n_a / MR_TSDF_BRICK) bricks per axis, x fastest.  With
 * B = MR_TSDF_BRICK the byte of brick (b_x, b_y, b_z) is 1 when some voxel with weight > min_weight and tsdf < 0 lies in
 * [B b_a, B b_a + B] on every axis (INCLUSIVE: one voxel of halo on the + side, because the corners of a cell reach i + 1), clipped to
 * the volume; otherwise 0.  One sweep of the volume, behind a clear of the bytes on the same stream.  Besides the volume cases of
 * mr_tsdf_volume_reset_f32: NaN min_weight, bricks NULL: MR_ERR_BAD_ARGUMENT, nothing is launched. */
int mr_tsdf_skip_grid_u8(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float min_weight, uint8_t* bricks,
                         void* stream);

/* One view of mr_tsdf_render_f32, passed by value in the launch arguments. */
typedef struct mr_tsdf_ray_view {
    float m[12];                 /* camera -> world, 3 x 4 row-major: R[a][j] = m[4a + j], c_a = m[4a + 3].  Nothing is inverted anywhere. */
    float fx, fy, cx, cy;        /* pixel intrinsics of the rendered image */
    float* depth;                /* height x width, device memory: camera-z metres, 0 = no surface */
    float* normal;               /* height x width x 3, device memory, may be NULL: unit normal in world axes, towards positive tsdf */
    uint8_t* colour;             /* height x width x 3 interleaved r g b, device memory, may be NULL; all 0 when the volume has no colour */
} mr_tsdf_ray_view;

/* Render views[0 .. num_views) (HOST array, 1 <= num_views <= MR_TSDF_MAX_FRAMES), all height x width, of the volume: the result equals
 * num_views launches of one view bit for bit.  All fp32, every operation rounded on its own:
 *   inv = 1 / voxel_size
 *   per view:   o_a = (c_a - origin_a) * inv
 *   per pixel (u, v):   rx = ((float)u - cx) / fx;  ry = ((float)v - cy) / fy
 *                       d_a = (R[a][0] * rx + R[a][1] * ry) + R[a][2];  e_a = d_a * inv
 *   sample k = 0, 1, ... while t_k <= t_max:
 *     t_k = t_min + (float)k * step
 *     g_a = o_a + t_k * e_a;  i_a = floorf(g_a);  f_a = g_a - i_a
 *     VALID iff 0 <= i_a and i_a + 1 <= n_a - 1 for all a, and the weights of all 8 corners i + {0, 1}^3 are > min_weight
 *     F_k = the trilinear interpolant of the 8 corner tsdf, every lerp in the form a + f * (b - a), along x, then y, then z
 *   state (prev_valid, F_prev), initially not valid, walked in the order of k:
 *     VALID and prev_valid and !(F_prev < 0) and  (F_k < 0)   HIT at k
 *     VALID and prev_valid and  (F_prev < 0) and !(F_k < 0)   the ray ends without a hit: it left the surface through a back face
 *     not VALID                                               prev_valid = false
 *     otherwise                                               prev = (valid, F_k)
 *   HIT:     s = F_prev / (F_prev - F_k);  depth = (t_min + (float)(k - 1) * step) + s * step
 *   no hit:  depth = 0, normal = 0 0 0, colour = 0 0 0
 * Normal and colour are taken in the cell and at the fractions f of sample k.  The normal is the analytic gradient of the interpolant:
 *   g_x = the lerp along z of the lerps along y of the four differences T[1][y][z] - T[0][y][z]           (T[x][y][z]: the corners)
 *   g_y = the lerp along z of the lerps along x of the four differences T[x][1][z] - T[x][0][z]
 *   g_z = the lerp along y of the lerps along x of the four differences T[x][y][1] - T[x][y][0]
 *   len = sqrtf((g_x * g_x + g_y * g_y) + g_z * g_z);  n = g / len if len > 0, else 0 0 0
 * in world axes, towards positive tsdf: out of the surface.  colour_c = (uint8)fminf(255, floorf(x + .5)), x the same trilinear
 * interpolant of the corners' bytes as floats.
 * bricks: NULL, or the bytes mr_tsdf_skip_grid_u8 wrote for THIS volume and THIS min_weight.  A sample whose cell base i lies in a
 * brick of byte 0 is not VALID, or VALID with F_k >= 0 (no corner is seen and negative, and a + f * (b - a) of non-negative a, b with
 * 0 <= f <= 1 is never negative in fp32), so it is neither a hit nor, unless F_prev < 0, the end of the ray; such samples cost one
 * byte load instead of 16 gathers, except that a sample is always evaluated in full while prev is valid and negative, and that the
 * sample before an evaluated one is evaluated in full as its prev.  The bricks change no bit of any output.  Rays are clipped to the
 * volume's box first, by a margin wider than fp32 can move a sample: samples outside it are not VALID anyway.
 * Besides the cases of mr_tsdf_extract_f32's volume: views NULL, num_views outside 1 .. MR_TSDF_MAX_FRAMES, a view without depth,
 * depth / normal off a 4-byte boundary, fx or fy 0 or NaN, height / width < 1, step <= 0 (or NaN), t_min < 0, t_max < t_min, either
 * not finite, more than 2^20 samples per ray, NaN min_weight: MR_ERR_BAD_ARGUMENT, nothing is launched. */
int mr_tsdf_render_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny, int32_t nz,
                       const float* origin, float voxel_size, float min_weight, const uint8_t* bricks, const mr_tsdf_ray_view* views,
                       int32_t num_views, int32_t height, int32_t width, float t_min, float t_max, float step, void* stream);

/* ---- A block-sparse TSDF volume (three entries added within ABI 24: the change only adds symbols; SparseTSDFVolume in
 * monorec_amd/tsdf_fusion.py): storage only for the blocks of MR_TSDF_BLOCK^3 = 8 x 8 x 8 voxels near a surface.  No hashing.
 *
 * The volume has nbx x nby x nbz BLOCKS, so 8 nbx x 8 nby x 8 nbz voxels; voxel (x, y, z) lies at p_a = origin_a + (float)i_a * voxel_size,
 * exactly as in the dense volume.
 *   table          int32[nbz * nby * nbx] in device memory, x fastest: -1 = the block has no storage, anything else is its slot.
 *                  nbx * nby * nbz < 2^31.
 *   pool           tsdf float[capacity * 512], weight float[capacity * 512], colour uint8[capacity * 512 * 4] or NULL.  Voxel
 *                  (lx, ly, lz) of slot s is at s * 512 + (lz * 8 + ly) * 8 + lx, a 64-bit index: every row of 8 voxels starts on a
 *                  32-byte boundary of a 16-byte aligned array, all accesses of the sweeps are 16 bytes wide, no ragged path exists.
 *   block_of_slot  int32[capacity]: the table index of each slot in use.
 *   cursor         one int64 in device memory, 0 on reset: the number of slot requests so far.  Slots 0 .. min(cursor, capacity) - 1
 *                  are in use; cursor > capacity: some block found no room (and still has none).
 * Reset: the table to -1 (a memset of 0xff), the cursor to 0.  The pool needs no clearing: a block is written in full when it gets a slot.
 *
 * mr_tsdf_sparse_integrate_f32: frames[0 .. num_frames) (HOST array, 1 <= num_frames <= MR_TSDF_MAX_FRAMES) as for mr_tsdf_integrate_f32.
 * For every block, within the one launch:
 *   1. start state: the pool's values if the block has a slot, otherwise tsdf 1, weight 0, colour 0 for every voxel;
 *   2. the frames in order into each of the 512 voxels, mr_tsdf_integrate_f32's arithmetic operation for operation (the same code),
 *      with the same skips, roundings and colour blend; a voxel is IN BAND when some frame updated it with diff / trunc < 1;
 *   3. the block has a slot: the touched voxels are stored, as by the dense kernel;
 *   4. no slot and no voxel in band: nothing is stored;
 *   5. no slot and some voxel in band: s = one fetch-add of 1 on *cursor; if s < capacity, table[b] = s, block_of_slot[s] = b and all 512
 *      voxels are stored (untouched ones as 1 / 0 / 0); otherwise nothing is stored.
 * So: WHICH slot a block gets is unspecified (the order of the workgroups); everything else is deterministic.  From the launch that
 * gives a block its slot on, the block's voxels equal those of a dense volume that was empty at the start of that launch and received
 * the same frames since: free-space observations (dist = 1) of EARLIER LAUNCHES are lost for that block, those of earlier frames of
 * the SAME launch are kept.  A block that never comes within trunc of an observed surface is never stored: it reads as unseen.
 * A workgroup owns one block.  It culls frames with the dense kernel's five planes against the block's bounding sphere and leaves
 * without touching memory, the table included, when no frame is live; the band decision is one workgroup-wide OR, the allocation one
 * atomic per new block.  The launch covers only the block-aligned box of the frames' frusta up to depth
 * min(max_depth_m, 327.67) + trunc (depths are int16 centimetres), computed here in double, pushed outwards like the planes and clipped
 * to the table: no voxel outside it could have been updated, so neither the box nor the culling changes a result, and a table of
 * millions of blocks costs nothing where no camera looks (no launch at all when the box misses the table).
 * MR_ERR_BAD_ARGUMENT, nothing is launched: every case of mr_tsdf_integrate_f32; table, block_of_slot or cursor NULL; capacity < 1 or
 * capacity * 512 >= 2^40; a block count < 1 or nbx * nby * nbz >= 2^31; tsdf / weight / colour off a 16-byte, cursor off an 8-byte,
 * table / block_of_slot off a 4-byte boundary. */
int mr_tsdf_sparse_integrate_f32(int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, float* tsdf, float* weight, uint8_t* colour,
                                 int32_t* block_of_slot, int64_t capacity, int64_t* cursor, const float* origin, float voxel_size,
                                 float trunc, float max_depth_m, const mr_tsdf_view* frames, int32_t num_frames, int32_t height,
                                 int32_t width, void* stream);

/* mr_tsdf_extract_f32's rule on the virtual dense volume of 8 nbx x 8 nby x 8 nbz voxels in which a block without a slot is unseen
 * (weight 0): as a set, the records equal those of mr_tsdf_extract_f32 on the gathered dense volume bit for bit.  num_slots: the slots
 * in use, min(cursor, capacity) of the integration, read by the caller; 0 launches nothing.  Cursor protocol (THIS cursor counts
 * records), record format and the count-only mode with records NULL are mr_tsdf_extract_f32's.  One workgroup per slot: it stages its
 * 8^3 voxels plus one beyond the high faces (9^3) from up to eight blocks through the table and leaves at the barrier when no seen
 * negative voxel is staged.  A table entry at or above num_slots reads as no slot.
 * MR_ERR_BAD_ARGUMENT: the table, pool and alignment cases above, origin NULL, voxel_size <= 0, NaN min_weight, num_slots < 0,
 * num_slots * 512 >= 2^40 or num_slots > nbx * nby * nbz, records off a 4-byte boundary, capacity_records < 0 with records. */
int mr_tsdf_sparse_extract_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf, const float* weight,
                               const uint8_t* colour, const int32_t* block_of_slot, int64_t num_slots, const float* origin,
                               float voxel_size, float min_weight, float* records, int64_t capacity_records, int64_t* cursor,
                               void* stream);

/* The box of dx x dy x dz voxels that starts at voxel (x0, y0, z0) of the sparse volume into dense arrays of the dense layout
 * (idx = (z * dy + y) * dx + x; out_colour 4 bytes per voxel, may be NULL): the pool's values, 1 / 0 / 0 where a block has no slot.
 * The box need not be block-aligned but must lie inside the volume.  MR_ERR_BAD_ARGUMENT: the table and pool cases above, out_tsdf or
 * out_weight NULL, out_colour without a pool colour, outputs off a 4-byte boundary, a negative offset, a size < 1, a box that leaves
 * the volume, dx * dy * dz >= 2^40. */
int mr_tsdf_sparse_gather_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf, const float* weight,
                              const uint8_t* colour, int32_t x0, int32_t y0, int32_t z0, int32_t dx, int32_t dy, int32_t dz,
                              float* out_tsdf, float* out_weight, uint8_t* out_colour, void* stream);

/* The sparse volume seen from a camera (added within ABI 24: the change only adds symbols).  The entry returns the result of
 * mr_tsdf_render_f32 with bricks NULL on the virtual dense volume of 8 nbx x 8 nby x 8 nbz voxels in which a block without a slot reads
 * tsdf 1, weight 0, colour 0 - what mr_tsdf_sparse_gather_f32 would write -: bit for bit, for depth, normal and colour, for every
 * min_weight and any number of views per launch.  The views, the samples t_k = t_min + (float)k * step, the VALID / HIT / back-face state
 * machine, the fp32 operation order and the 2^20-sample cap are mr_tsdf_render_f32's (the same code, csrc/tsdf_render.h).
 * num_slots: the slots in use, as for mr_tsdf_sparse_extract_f32; a table entry below 0 or at or above num_slots is no slot.
 * num_slots == 0 is no error: no voxel is negative, every output is written as 0.
 * Corner fetch: for the cell base i, corner i + d lies in block (i + d) >> 3 at the local voxel (i + d) & 7, pool index
 * slot * 512 + (lz * 8 + ly) * 8 + lx (64 bit).  When (i_a & 7) < 7 on all three axes - 343 of every 512 cells - the eight corners share
 * one block and one table load serves them; otherwise up to eight table loads.  A corner in a block without a slot yields weight 0,
 * tsdf 1, colour 0 without touching the pool.
 * Empty space: with min_weight >= 0 a sample whose base cell lies in a block without a slot is not VALID (corner i itself has weight 0):
 * it costs one table load and sets prev_valid = false.  With min_weight < 0 such corners count as seen with tsdf 1 and the sample is
 * evaluated in full, with no shortcut.
 * MR_ERR_BAD_ARGUMENT, nothing is launched: the table, pool and alignment cases of the other sparse entries; a block count above 2^27 on
 * some axis; num_slots < 0, num_slots * 512 >= 2^40 or num_slots > nbx * nby * nbz; origin NULL, voxel_size <= 0 (or NaN), NaN
 * min_weight; every view, size and range case of mr_tsdf_render_f32. */
int mr_tsdf_sparse_render_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf, const float* weight,
                              const uint8_t* colour, int64_t num_slots, const float* origin, float voxel_size, float min_weight,
                              const mr_tsdf_ray_view* views, int32_t num_views, int32_t height, int32_t width, float t_min, float t_max,
                              float step, void* stream);

/* The sparse volume as a welded triangle mesh (two entries added within ABI 24: the change only adds symbols).  As canonical meshes -
 * vertices as a set, triangles as a set of triples of vertices - the result equals that of mr_tsdf_mesh_vertices_f32 and
 * mr_tsdf_mesh_triangles_f32 on the virtual dense volume of 8 nbx x 8 nby x 8 nbz voxels in which a block without a slot is UNSEEN
 * whatever min_weight is: bit for bit, records, masks, tetrahedra, parity and winding by the same code (csrc/tsdf_common.h,
 * csrc/tsdf_mesh.h).  With min_weight >= 0 that volume is the gathered one (mr_tsdf_sparse_gather_f32 writes weight 0 there).  The one
 * difference: with min_weight < 0 the gathered volume's empty blocks count as seen with tsdf 1 and the dense entries put a surface
 * between them and every negative voxel next to them; here they stay unseen and that surface is absent, as for
 * mr_tsdf_sparse_extract_f32.
 * Slots: num_slots as for mr_tsdf_sparse_extract_f32; 0 launches nothing.  A table entry below 0 or at or above num_slots is no slot, a
 * neighbour beyond the table is unseen.  One workgroup per slot, which owns the vertices of its block's voxels and the triangles of the
 * cubes whose base voxel lies in its block; a cube with a corner in a block without a slot emits nothing, so iterating over the slots
 * is complete.  A workgroup that stages no seen negative voxel (its block and what it reaches of the seven + neighbours) touches neither
 * its output, nor vertex_base, nor the cursor.
 * vertex_base: int32[num_slots * 512], caller-owned, indexed like the pool - voxel (lx, ly, lz) of slot s at s * 512 + (lz * 8 + ly) * 8
 * + lx, a 64-bit index; only the values are int32.  Its size follows the pool, not the dense box.  The vertex entry writes the index of
 * the first vertex of every voxel that owns one and leaves the rest untouched; index(v, e) = vertex_base[v] + popcount(mask(v) &
 * ((1 << e) - 1)) as in the dense mesh.  The triangle entry recomputes the masks from the same table, pool, num_slots and min_weight and
 * reads vertex_base in the owner's own slot - across a block face that of a + neighbour.
 * Positions are origin_a + (float)(8 b_a + l_a) * voxel_size, as mr_tsdf_sparse_extract_f32 computes them: the vertices on axis edges are
 * its records.  Cursor protocol, capacity rule (counted, not written, at or beyond the capacity) and the count-only mode (vertices /
 * triangles NULL: capacity and vertex_base are ignored, vertex_base may be NULL) are the dense mesh entries'.  Indices are int32: a
 * caller whose vertex count reaches 2^31 must not fill.
 * MR_ERR_BAD_ARGUMENT, nothing is launched: the table, pool and alignment cases of mr_tsdf_sparse_extract_f32 (the triangle entry has
 * neither colour nor origin nor voxel_size); num_slots < 0, num_slots * 512 >= 2^40 or num_slots > nbx * nby * nbz; NaN min_weight;
 * vertex_base / vertices / triangles off a 4-byte boundary; an output without vertex_base; a negative capacity with an output. */
int mr_tsdf_sparse_mesh_vertices_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf, const float* weight,
                                     const uint8_t* colour, const int32_t* block_of_slot, int64_t num_slots, const float* origin,
                                     float voxel_size, float min_weight, float* vertices, int64_t capacity_vertices,
                                     int32_t* vertex_base, int64_t* cursor, void* stream);
int mr_tsdf_sparse_mesh_triangles_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf, const float* weight,
                                      const int32_t* block_of_slot, int64_t num_slots, float min_weight, const int32_t* vertex_base,
                                      int32_t* triangles, int64_t capacity_triangles, int64_t* cursor, void* stream);

/* Vertex normals and a clustered level of detail for both meshes (six entries added within ABI 24: the change only adds symbols).
 * Everything is fp32, every operation rounded on its own; tests/tsdf_mesh_lod_ref.py restates it in numpy.  No float atomics.
 *
 * Normals.  A voxel is SEEN when it lies inside the volume, has weight > min_weight and - in the sparse volume - its block has a slot
 * below num_slots.  For a seen voxel v and an axis i
 *   g_i[v] = hi - lo,  hi = tsdf[v + e_i] if that voxel is seen, else tsdf[v];  lo = tsdf[v - e_i] if that voxel is seen, else tsdf[v]
 * The vertex on the active edge from a = v to b = v + d_e, at the parameter s = tsdf[a] / (tsdf[a] - tsdf[b]) of its position, has
 *   m_i = g_i[a] + s * (g_i[b] - g_i[a]);  len = sqrtf((m_0 * m_0 + m_1 * m_1) + m_2 * m_2);  normal_i = m_i / len if len > 0, else 0
 * Tsdf grows from the inside to the outside, so the normal points where (b - a) x (c - a) of the triangles points.
 * The two _normals_ entries are mr_tsdf_mesh_vertices_f32 and mr_tsdf_sparse_mesh_vertices_f32 - the same tile code, records, order,
 * vertex_base and cursor - that also write normal x y z of the vertex with index i to normals[3 i .. 3 i + 3).  normals may be NULL only
 * when vertices is; it needs a 4-byte boundary and room for 3 floats per vertex below the capacity.
 *
 * Clusters.  With c = cell in {2, 4, 8}, cluster (X, Y, Z) holds the voxels with x / c = X, y / c = Y, z / c = Z (integer division);
 * the dense volume has ceil(n_a / c) clusters per axis - partial ones on the high side where c does not divide n_a -, a block of the
 * sparse volume (8 / c)^3.  A cluster that owns at least one vertex of the full mesh - one of its voxels has a mask other than 0 -
 * emits ONE vertex.  Its members are visited in one fixed order: the cluster's voxels with z outermost, then y, x fastest - voxel
 * i = (dz * c + dy) * c + dx -, within a voxel its active edges e = 0 .. 6.  The sum is a tree of a fixed shape: the voxels are cut
 * into RUNS of 8 in that order, run r = i / 8 (a cluster of 2^3 is one run, of 4^3 eight runs of two rows, of 8^3 sixty-four runs of
 * one row).  Over the six floats of a member's record and the three of its normal (as above):
 *   run_k[r] starts at 0.0f and takes run_k[r] = run_k[r] + value_k per member of run r, in the order above (one lane per run)
 *   sum_k starts at 0.0f and takes sum_k = sum_k + run_k[r] for r = 0, 1, ... (one lane per cluster; a run without a member adds 0.0f)
 *   record_k = sum_k / (float)count  for x y z red green blue (the colours are NOT rounded again)
 *   len = sqrtf((sum_nx * sum_nx + sum_ny * sum_ny) + sum_nz * sum_nz);  normal = sum_n / len if len > 0, else 0
 * Every triangle of the full mesh is mapped to the clusters of the owner voxels of its three vertices (corners c0, c1, c2 of its
 * tetrahedron).  If two of the three clusters coincide the triangle is dropped; the others are written with their winding kept, as three
 * indices of cluster vertices.  Triangles that repeat are kept.
 * cluster_base: int32, caller-owned.  Dense: one element per cluster, ((Z * cy) + Y) * cx + X with c_a = ceil(n_a / c).  Sparse:
 * (8 / c)^3 per slot, s * (8 / c)^3 + ((Z * (8 / c)) + Y) * (8 / c) + X with the cluster's place in its block.  The vertex entry writes
 * the vertex index of every cluster that owns a vertex and leaves the rest untouched; the triangle entry recomputes cases and clusters
 * from the same volume and min_weight and reads it - across a block face in the slot of a + neighbour.
 * Workgroups: the dense vertex entry gives a workgroup MR_TSDF_CLUSTER_TILE_X x _Y x _Z voxels - whole clusters for every c -, the
 * sparse one a slot; the triangle entries use the tile of mr_tsdf_mesh_triangles_f32 and a slot.  Cursor protocol (one atomicAdd per
 * workgroup), capacity rule and the count-only mode (vertices / triangles NULL: capacity, normals and cluster_base are ignored) are the
 * mesh entries'.  normals NULL with vertices: no normals are computed.
 * MR_ERR_BAD_ARGUMENT, nothing is launched: every case of the mesh entries of the same volume, with cluster_base in the place of
 * vertex_base; a cell other than 2, 4 or 8; normals off a 4-byte boundary; normals without vertices (for the _normals_ entries also
 * vertices without normals); nz > 2^31 - 10 (dense vertex entry); num_slots * (8 / c)^3 >= 2^31 (sparse). */
#define MR_TSDF_CLUSTER_TILE_X 32
#define MR_TSDF_CLUSTER_TILE_Y 8
#define MR_TSDF_CLUSTER_TILE_Z 8
int mr_tsdf_mesh_vertices_normals_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny, int32_t nz,
                                      const float* origin, float voxel_size, float min_weight, float* vertices, int64_t capacity_vertices,
                                      float* normals, int32_t* vertex_base, int64_t* cursor, void* stream);
int mr_tsdf_mesh_cluster_vertices_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny, int32_t nz,
                                      const float* origin, float voxel_size, float min_weight, int32_t cell, float* vertices,
                                      int64_t capacity_vertices, float* normals, int32_t* cluster_base, int64_t* cursor, void* stream);
int mr_tsdf_mesh_cluster_triangles_f32(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float min_weight,
                                       int32_t cell, const int32_t* cluster_base, int32_t* triangles, int64_t capacity_triangles,
                                       int64_t* cursor, void* stream);
int mr_tsdf_sparse_mesh_vertices_normals_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf,
                                             const float* weight, const uint8_t* colour, const int32_t* block_of_slot, int64_t num_slots,
                                             const float* origin, float voxel_size, float min_weight, float* vertices,
                                             int64_t capacity_vertices, float* normals, int32_t* vertex_base, int64_t* cursor, void* stream);
int mr_tsdf_sparse_mesh_cluster_vertices_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf,
                                             const float* weight, const uint8_t* colour, const int32_t* block_of_slot, int64_t num_slots,
                                             const float* origin, float voxel_size, float min_weight, int32_t cell, float* vertices,
                                             int64_t capacity_vertices, float* normals, int32_t* cluster_base, int64_t* cursor, void* stream);
int mr_tsdf_sparse_mesh_cluster_triangles_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf,
                                              const float* weight, const int32_t* block_of_slot, int64_t num_slots, float min_weight,
                                              int32_t cell, const int32_t* cluster_base, int32_t* triangles, int64_t capacity_triangles,
                                              int64_t* cursor, void* stream);

/* ---- input pipeline: KittiOdometryDataset.preprocess_image, kitti_odometry_dataset.py:120-134 ------
 *
 * img.crop(box) -> img.resize((W,H), Image.BILINEAR) -> float32 / 255 - .5 -> CHW (a 1-channel image is stacked 3x),
 * Pillow's resampling (Resample.c: scaled triangle filter, 22-bit fixed-point weights, horizontal pass into an 8-bit
 * intermediate, then vertical) reproduced bit for bit.
 *
 * Host side, once per (size, box): the coefficient tables of one axis for a crop [in0, in1) of an axis of in_size
 * pixels resized to out_size.  ksize = mr_resample_ksize_bilinear(in0, in1, out_size); bounds: out_size x 2 ints
 * (first source index, tap count), coeffs: out_size x ksize ints (unused taps 0).  For a cropped image pass
 * in_size = in1 - in0, in0 = 0 (Image.crop materialises the crop before the resize). */
int32_t mr_resample_ksize_bilinear(int32_t in0, int32_t in1, int32_t out_size);
int mr_resample_coeffs_bilinear(int32_t in_size, int32_t in0, int32_t in1, int32_t out_size, int32_t* bounds,
                                int32_t* coeffs);

/* Device side: src = decoded image in device memory, uint8, interleaved (src_h, src_w, channels), channels 1 or 3;
 * box = integer crop (x0, y0, x1, y1) as Image.crop rounds it; tables (device memory) for the cropped size;
 * max_tile_rows = max over output row tiles [16t, 16t+16) of the source rows they touch
 * (vbounds[last].first + vbounds[last].count - vbounds[first].first); dst (3, out_h, out_w) fp32. */
int mr_preprocess_image_u8_f32(const uint8_t* src, int32_t src_h, int32_t src_w, int32_t channels,
                               int64_t row_stride_bytes, const int32_t* box, int32_t out_h, int32_t out_w,
                               const int32_t* hbounds, const int32_t* hcoeffs, int32_t hksize,
                               const int32_t* vbounds, const int32_t* vcoeffs, int32_t vksize,
                               int32_t max_tile_rows, float* dst, void* stream);

/* The same launch with a photometric response table between the resize and the division: TUMMonoVODataset.preprocess_image
 * (tum_mono_vo_dataset.py:84-100), dst = lut256[8-bit result of the resize] / 255 - .5.  lut256: 256 floats in device memory
 * (the inverse response of the sequence, invert_pcalib, :247-254), held in the LDS during the launch.  A 1-channel source is
 * resized once and written to the three planes (`convert('RGB')` first gives the same bytes).
 * lut256 == NULL: MR_ERR_BAD_ARGUMENT. */
int mr_preprocess_image_u8_lut_f32(const uint8_t* src, int32_t src_h, int32_t src_w, int32_t channels,
                                   int64_t row_stride_bytes, const int32_t* box, int32_t out_h, int32_t out_w,
                                   const int32_t* hbounds, const int32_t* hcoeffs, int32_t hksize,
                                   const int32_t* vbounds, const int32_t* vcoeffs, int32_t vksize,
                                   int32_t max_tile_rows, const float* lut256, float* dst, void* stream);

/* ---- pre-decoded frame store (monorec_amd/frame_store.py): what the three launches above produce, kept as bytes on disk ----
 *
 * Write side.  The launch of mr_preprocess_image_u8_f32 (kitti_odometry_dataset.py:120-134) stopped after the resize: the 8-bit
 * value of the vertical pass, before table, division and grey replication, to `channels` planes of out_h x out_w bytes, plane p
 * at dst + p * plane_stride (plane_stride >= out_h * out_w bytes, else MR_ERR_BAD_ARGUMENT). */
int mr_preprocess_image_u8_u8(const uint8_t* src, int32_t src_h, int32_t src_w, int32_t channels,
                              int64_t row_stride_bytes, const int32_t* box, int32_t out_h, int32_t out_w,
                              const int32_t* hbounds, const int32_t* hcoeffs, int32_t hksize,
                              const int32_t* vbounds, const int32_t* vcoeffs, int32_t vksize,
                              int32_t max_tile_rows, uint8_t* dst, int64_t plane_stride, void* stream);

/* Read side.  The rest of preprocess_image on stored bytes (kitti_odometry_dataset.py:120-134; with a table
 * tum_mono_vo_dataset.py:92-94): src = `channels` (1 or 3) planes of h x w bytes in device memory, 16-byte aligned, plane p at
 * src + p * plane_stride; dst (3, h, w) fp32 = (lut256 ? lut256[u] : u) / 255 - .5, a 1-plane source written to all three planes.
 * lut256: 256 floats in device memory or NULL.  plane_stride % 16 != 0 or plane_stride < h * w: MR_ERR_BAD_ARGUMENT. */
int mr_unpack_frame_u8_f32(const uint8_t* src, int32_t channels, int64_t plane_stride, int32_t h, int32_t w,
                           const float* lut256, float* dst, void* stream);

/* A stored sparse target back on its grid: the keyframe_depth of kitti_odometry_dataset.py:226-246 (annotated lidar :184-211,
 * D(V)SO :156-182) kept as its non-zero cells.  dst (cells floats) is zero-filled, then dst[index[i]] = value[i] for i < n;
 * indices are unique, one >= cells is skipped; n == 0 is valid (index / value may then be NULL). */
int mr_scatter_sparse_f32(const uint32_t* index, const float* value, int64_t n, float* dst, int64_t cells, void* stream);

/* Sparse lidar ground truth, preprocess_depth_annotated_lidar (kitti_odometry_dataset.py:184-211): the 16-bit depth PNG
 * (depth * 256, 0 = no return) -> inverse depth 256 / value scattered to the nearest cell of the (out_h, out_w) grid of
 * the cropped (box = x0, y0, x1, y1; NULL = none) and rescaled image; colliding samples: last one in row-major source
 * order wins, like numpy's fancy assignment.  owner_scratch: out_h * out_w ints of device scratch.  dst (out_h, out_w). */
int mr_lidar_inverse_depth_u16_f32(const uint16_t* depth_png, int32_t src_h, int32_t src_w, const int32_t* box,
                                   int32_t out_h, int32_t out_w, int32_t* owner_scratch, float* dst, void* stream);

/* Sparse D(V)SO ground truth, preprocess_depth_dso (kitti_odometry_dataset.py:156-182): the 16-bit PNG (0 = no point) ->
 * inverse depth orig_w * value / (0.54 * focal_x * 65535) scattered like mr_lidar_inverse_depth_u16_f32; source coordinates
 * are rescaled to the original image size (orig_h, orig_w) first and the crop box is tested on those (NULL = none). */
int mr_dso_inverse_depth_u16_f32(const uint16_t* depth_png, int32_t src_h, int32_t src_w, int32_t orig_h, int32_t orig_w,
                                 double focal_x, const int32_t* box, int32_t out_h, int32_t out_w,
                                 int32_t* owner_scratch, float* dst, void* stream);

int mr_abi_version(void);
const char* mr_error_string(int code);

#ifdef __cplusplus
}
#endif
#endif /* MONOREC_HIP_H */
