// Internal declarations shared by the host executor and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/uda_hip.h"

namespace uda {

// ---------------------------------------------------------------- counter-based random stream (shared with oracle/philox_ref.py)
#ifdef __HIPCC__
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// One standard-normal draw per (i0, i1, i2) of stream `tag`: words of Philox4x32-10(counter = (i0, i1, i2, tag), key = seed),
// u1 = ((w0 >> 8) + 0.5) 2^-24 in (0, 1), u2 = (w1 >> 8) 2^-24, z = sqrt(-2 ln u1) cos(2 pi u2) in float64 (Box-Muller).
// Used where the reference draws from TFP distributions (class-calibration logit samples, utils_class.py:121-123; the
// `sample` decode, utils_box.py:162-184): TF's stream cannot be reproduced, so the build defines this one.
__device__ __forceinline__ double philox_normal(uint64_t seed, uint32_t i0, uint32_t i1, uint32_t i2, uint32_t tag) {
  uint32_t w[4];
  philox4x32_10(i0, i1, i2, tag, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  const double u1 = ((double)(w[0] >> 8) + 0.5) * 5.9604644775390625e-08;
  const double u2 = (double)(w[1] >> 8) * 5.9604644775390625e-08;
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
}
// both Box-Muller values of one Philox call: z0 = r cos(2 pi u2), z1 = r sin(2 pi u2)
__device__ __forceinline__ void philox_normal2(uint64_t seed, uint32_t i0, uint32_t i1, uint32_t i2, uint32_t tag, double& z0, double& z1) {
  uint32_t w[4];
  philox4x32_10(i0, i1, i2, tag, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  const double u1 = ((double)(w[0] >> 8) + 0.5) * 5.9604644775390625e-08;
  const double u2 = (double)(w[1] >> 8) * 5.9604644775390625e-08;
  const double r = sqrt(-2.0 * log(u1)), th = 6.283185307179586476925286766559 * u2;
  z0 = r * cos(th);
  z1 = r * sin(th);
}

// The activations of utils.activation_fn (reference utils.py:42-59) other than swish, which every kernel keeps as its own
// first branch (`act == UDA_ACT_SWISH`): relu = max(x, 0), relu6 = min(max(x, 0), 6), hswish = x * relu6(x + 3) / 6.
// One clamp with two wave-uniform constants (+ a multiply for hswish; the division by six is a multiplication by its
// float32 reciprocal, 1 ulp like the hardware rcp / exp2 of the swish path): four vector instructions and no live register
// beyond the value, so the epilogues of the tuned kernels keep their register counts (tools/codeobj.py resources).
__device__ __forceinline__ float act_relu_family(float v, int act) {
  if (act == UDA_ACT_MISH) {
    // x tanh(softplus(x)) = x n / (n + 2) with n = e^x (e^x + 2): one exp, one rcp (the hardware ones, as in the swish path);
    // beyond x = 20 the quotient is 1 to float32 and e^2x would overflow
    const float e = __expf(fminf(v, 20.0f));
    const float n = e * (e + 2.0f);
    return v * (n * __builtin_amdgcn_rcpf(n + 2.0f));
  }
  const float off = act == UDA_ACT_HSWISH ? 3.0f : 0.0f;
  const float hi = act == UDA_ACT_RELU ? __builtin_inff() : 6.0f;
  const float r = __builtin_amdgcn_fmed3f(v + off, 0.0f, hi);
  return act == UDA_ACT_HSWISH ? (v * r) * 0.16666667163372040f : r;
}
#endif

// An executor knob of the environment (A/B switches, test hooks; DESIGN.md 7 lists them): the integer value of `name`, `dflt` when
// unset.  Call sites keep the result in a function-local static, i.e. read it once per process.
static inline int uda_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// ---------------------------------------------------------------- split-precision schemes of the 1x1 contractions
// (`wparts` of the argument blocks below = PARTS of the kernels; see mfma_common.h): enum uda_pw_scheme of uda_hip.h
inline bool uda_split_one(int scheme) { return scheme == UDA_SPLIT_F16X1 || scheme == UDA_SPLIT_BF16X1; }   // one piece per operand, one product
inline int uda_split_pieces(int scheme) { return scheme == UDA_SPLIT_BF16X3 ? 3 : (uda_split_one(scheme) ? 1 : 2); }
inline bool uda_split_f16(int scheme) { return scheme == UDA_SPLIT_F16X2 || scheme == UDA_SPLIT_F16X1; }   // fp16 pieces: range-tracked

// ---------------------------------------------------------------- kernel argument blocks
struct PreGeo;
struct StemArgs {
  const float* in;    // [rows, H, W, 3]
  float* out;         // [rows, Ho, Wo, Co]
  const float* w;     // [27, Co]
  const float* bn_scale;
  const float* bn_shift;
  int H, W, Ho, Wo, Co;
  int pad_t, pad_l;
  int rows;
  // uint8 input (every image of the batch at scale 1: nothing to resample): the stem normalises on the fly through a 768-entry
  // table of ((float)v - mean[c]) / std[c] - the preprocess kernel's own expression, so the convolution sees the same values bit
  // for bit - and reads a quarter of the bytes; the separate preprocess pass and its float32 image are skipped
  const uint8_t* u8;  // packed raw images (image i at u8 + geo[i].off, [geo[i].h, geo[i].w, 3]) or null
  const PreGeo* geo;  // [images] (device)
  int img0;           // first image of this launch in geo
  float mean[3], stdv[3];
  int act;            // uda_act (the specialised stems are swish kernels: any other activation runs stem_kernel)
};

struct PwArgs {
  const float* in;       // [rows_in, HW, Cin]
  float* out;            // [rows, HW, Cout]
  int in_f16;            // one piece only: `in` holds 16-bit values of the scheme's format, fp16 or bf16 (the expanded tensor of a fused MBConv front half)
  const float* w;        // [Cin, Cout]
  const float* bias;     // [Cout] or null
  const float* bn_scale; // [Cout] or null
  const float* bn_shift;
  const float* se;       // [rows / se_div, Cin] gate on the input or null
  const float* mask;     // [rows, Cout] dropout keep-scale or null
  const float* res;      // [rows, HW, Cout] residual or null
  int HW, Cin, Cout;
  int in_div;            // rows_in = rows / in_div (input shared by the MC samples of an image)
  int res_div;
  int se_div;            // 1: one gate per output row (per sample); in_div: one per input row
  int act;
  const void* wsplit;    // split weights in MFMA fragment order (kernels_pwb.hip) or null
  int wparts;            // split scheme of wsplit (UDA_SPLIT_*)
  float wunscale;        // the packed weights are the kernel times 1 / wunscale (a power of two; 1 unless fp16 pieces)
  unsigned* oor;         // fp16 pieces: word that receives bit 0 when an operand above 65504 was split (or null)
};
void launch_pwb(const PwArgs& a, int rows, hipStream_t s);
size_t pwb_packed_elems(int K, int N, int scheme);
// scale: every weight is multiplied by it before the split (a power of two; fp16 pieces only)
void pwb_pack_weights(const float* w, int K, int N, int scheme, uint16_t* out, float scale = 1.0f);
// power of two that brings the largest magnitude of w[0 .. n) into [2^13, 2^14) (1 for an all-zero tensor)
float split_weight_scale(const float* w, size_t n);

struct SepArgs {          // fused depthwise 3x3 (stride 1, SAME) + 1x1 (kernels_pwb.hip)
  const float* in;        // [rows / in_div, H, W, C]
  float* out;             // [rows, H, W, Cout]
  const float* wd;        // depthwise kernel [9, C]
  const void* wsplit;     // 1x1 kernel [C, Cout] as split-bf16 fragments
  const float* bias;      // [Cout] or null
  const float* bn_scale;  // [Cout] or null
  const float* bn_shift;
  const float* mask;      // [rows, Cout] dropout keep-scale or null
  const float* mask_in;   // [rows, C] DEFERRED keep-scale of the input channels (the producer left its dropout site to this op:
                          // input shared by the in_div samples of an image; sep_kernel's TIN mode) or null
  int H, W, C, Cout;
  int in_div;
  int act;
  int wparts;             // split scheme (UDA_SPLIT_*)
  float wunscale;         // see PwArgs
  unsigned* oor;
};
// rows = sample rows of the output; with mask_in the grid runs over rows / in_div images and each block serves the in_div samples
void launch_sep(const SepArgs& a, int rows, hipStream_t s);
bool sep_tin_supported(int C, int Cout, int scheme);      // the deferred-input mode exists for this shape (plan.py mirrors it)
// Several independent separable convs of ONE shape class (same C, Cout, activation, sample-axis relation, row count) in one
// launch: the five pyramid levels of a head layer.  The grid covers the tiles of all problems; a block finds its problem
// from the tile prefix sums.  Everything that differs between the problems lives in SepLevel.
constexpr int UDA_SEP_MAX_LV = 8;
struct SepLevel {
  const float* in; float* out; const float* wd; const void* wsplit;
  const float* bias; const float* bn_scale; const float* bn_shift; const float* mask; const float* mask_in;
  int H, W;
  float wunscale;
};
struct SepMulti {
  SepArgs one;                         // the single problem (n_lv == 0) / the fields shared by all problems
  int n_lv;
  int tiles, rows;                     // tiles of one sample row (all problems), sample rows: filled by the launcher
  int tile0[UDA_SEP_MAX_LV + 1];       // first tile of every problem, total in [n_lv]
  SepLevel lv[UDA_SEP_MAX_LV];
};
void launch_sep_multi(const SepArgs& common, const SepLevel* lv, int n_lv, int rows, hipStream_t s);
bool sep_supported(int C, int Cout);
size_t sep_lds_bytes(int C, int Cout, int scheme, bool tin = false);      // dynamic LDS of the launch an op of this shape gets
struct FuseArgs;
// The same conv on an LDS-staged 16 x 16 tile (kernels_sep.hip: sepf_kernel) whose input is the BiFPN fusion described by
// `fused`, computed on the fly (a.in unused).
void launch_sepf(const SepArgs& a, const FuseArgs& fused, int rows, hipStream_t s);
bool sepf_supported(int C, int Cout, int scheme);
size_t sepf_lds_bytes(int C, int Cout, int scheme);

struct DwArgs {
  const float* in;       // [rows_in, H, W, C]
  float* out;            // [rows, Ho, Wo, C]
  const float* w;        // [k*k, C]
  const float* bn_scale; // or null
  const float* bn_shift;
  const float* mask;     // [rows, C] or null
  float* se_partial;     // [rows, n_tiles, C] or null
  int H, W, Ho, Wo, C;
  int pad_t, pad_l;
  int in_div;
  int act;
  int tc;                // threads along channel quads
  int pxb;               // x-groups per block
  int n_cchunk;          // channel chunks (grid.z = rows * n_cchunk)
  int n_tiles;           // Ho * gridDim.x
};

struct MbxArgs {
  const float* in;        // [rows_in, H, W, Cin]
  float* out;             // [rows, Ho, Wo, Cmid]
  int out_f16;            // one piece only: `out` is stored in the scheme's 16-bit format, fp16 or bf16 (round to nearest; the SE tile sums stay float32)
  const float* we;        // expand kernel [Cin, Cmid]
  const float* sc0;       // BN after expand
  const float* sh0;
  const float* mask0;     // [rows, Cmid] or null
  const float* wd;        // depthwise kernel [k*k, Cmid]
  const float* sc1;       // BN after depthwise
  const float* sh1;
  const float* mask1;     // [rows, Cmid] or null
  float* se_partial;      // [rows, n_tiles, Cmid] or null
  int H, W, Ho, Wo, Cin, Cmid;
  int pad_t, pad_l;
  int in_div;
  int n_tiles;
  const void* wsplit;     // expand kernel * BN scale (+ BN shift row) as split fragments (kernels_pwb.hip) or null
  int wparts;             // split scheme of wsplit (UDA_SPLIT_*)
  unsigned* oor;          // fp16 pieces: out-of-range flag word (see PwArgs) or null
  const float* wpar;      // per-slab depthwise taps + BN scale / shift block (mbx_pack_params) or null
  // fused projection of the previous block (mbxb_kernel FUSE0): in = D [rows / in_div, H, W, c0]
  const float* gate;      // [rows / g_div, c0] per-sample gate on D (SE gate x deferred dropout), null = not fused
  const float* w0t;       // [32][32] projection kernel^T x BN scale (mbxb_pack_proj)
  const float* sh0f;      // [32] projection BN shift
  const uint4* w0frag;    // [rows / g_div][2 k-steps][wparts][64 lanes]: W0^T x gate, split, in A-fragment order (launch_w0gate) or null
  int c0, g_div;
  // block order of launches whose input is shared by the in_div samples of an image (mbxb_kernel): 1-D grid, the
  // in_div blocks of one tile adjacent and on ONE XCD (ids = tile slot + 8 t), so that the shared tile is fetched into
  // that XCD's L2 once instead of once per sample; 0 = plain (tiles_x, tiles_y, rows) grid
  int remap_T, tiles_x, tiles_y;
  // deep variants (mbxd / mbxp) on small grids (a few sample rows): the 32-channel slabs of a tile are divided among
  // ch_groups blocks (grid z = rows x ch_groups), so that a launch of fewer blocks than the device holds still fills it
  int ch_groups;
};
void mbxb_pack_proj(const float* w0, const float* sc, const float* sh, int c0, int cout, float* out);
size_t mbx_par_floats(int Cmid, int k);
void mbx_pack_params(const float* wd, const float* sc1, const float* sh1, int Cmid, int k, float* out);
void launch_mbxb(const MbxArgs& a, int rows, int k, int stride, hipStream_t s);
void launch_mbxd(const MbxArgs& a, int rows, int k, int stride, hipStream_t s);     // deep blocks (Cin > 48), stride 1 or 2
bool mbxd_supported(int Cin, int Cmid, int k, int stride);
size_t mbx_lds_bytes(int Cin, int Cmid, int k, int stride, int scheme, int Ho, int Wo);   // dynamic LDS of the fused launch of this op
int mbxd_tiles(int Ho, int Wo, int k, int stride = 1);
bool mbxd_wide(int Ho, int Wo, int k, int stride);     // 20-column tiles for this map (mirror: plan.mbx_tile)
bool mbxb_supported(int Cin, int Cmid, int k, int stride);
int mbxb_tiles(int Ho, int Wo, int k, int stride);
size_t mbxb_packed_elems(int Cin, int Cmid, int scheme = UDA_SPLIT_BF16X2);
size_t mbxb_w0frag_elems(int gate_rows, int scheme);
void launch_w0gate(const float* gate, const float* w0t, int c0, int gate_rows, int scheme, uint4* out, unsigned* oor, hipStream_t s);
// stats (optional, 2 floats): largest magnitude and rms of the matrix that was packed (expand kernel x BN scale, shift row)
void mbxb_pack_weights(const float* we, const float* sc0, const float* sh0, int Cin, int Cmid, uint16_t* out, bool perm16 = false,
                       int scheme = UDA_SPLIT_BF16X2, float* stats = nullptr);
void launch_mbx(const MbxArgs& a, int rows, int k, int stride, hipStream_t s);
int mbx_tiles(int Ho, int Wo, int k, int stride);
bool mbx_supported(int Cin, int Cmid, int k, int stride);

struct SeArgs {
  const float* partial;  // [rows, n_tiles, C]
  float* scale;          // [rows, C]
  const float* w1;       // [C, mid]
  const float* b1;       // [mid]
  const float* w2;       // [mid, C]
  const float* b2;       // [C]
  int C, mid, n_tiles;
  float inv_hw;
  const float* mask;     // [rows, C] deferred dropout keep-scale of the squeezed tensor, or null
  int in_div;            // partial sums are per input row: rows / in_div
  int act;               // uda_act of the reduce layer (relu_fn, efficientnet_model.py:225)
};

struct FuseArgs {
  const float* in[UDA_MAX_FUSE_INPUTS];
  float* out;
  float wgt[UDA_MAX_FUSE_INPUTS];
  int mode[UDA_MAX_FUSE_INPUTS];   // uda_resample
  int Hi[UDA_MAX_FUSE_INPUTS], Wi[UDA_MAX_FUSE_INPUTS];
  int in_div[UDA_MAX_FUSE_INPUTS];
  float sy[UDA_MAX_FUSE_INPUTS], sx[UDA_MAX_FUSE_INPUTS];       // nearest: in/out
  int pk[UDA_MAX_FUSE_INPUTS], ps[UDA_MAX_FUSE_INPUTS];         // pool size / stride
  int ppt[UDA_MAX_FUSE_INPUTS], ppl[UDA_MAX_FUSE_INPUTS];       // pool pad before
  int n_in;
  int H, W, C;
  int act;
  int64_t total;  // rows*H*W*C/4
};

// ---------------------------------------------------------------- launchers (kernels_conv.hip)
void launch_stem(const StemArgs& a, hipStream_t s);
bool stem_u8_supported(int Co);      // the uint8-input variant of the stem exists for this width
void launch_pw(const PwArgs& a, int rows, hipStream_t s);
void launch_dw(DwArgs a, int rows, int k, int stride, hipStream_t s);
void dw_geometry(int C, int Wo, int k, int stride, int* tc, int* pxb, int* n_cchunk, int* grid_x, int* xb);
int dw_tiles(int C, int Ho, int Wo, int k, int stride);  // SE tile sums one depthwise launch leaves per sample row
void launch_se(const SeArgs& a, int rows, hipStream_t s);
void launch_fuse(const FuseArgs& a, hipStream_t s);
void launch_philox_masks(float* masks, const int64_t* site_off_dev, const int32_t* site_ch_dev,
                         const float* site_rate_dev, int n_sites, int rows, uint32_t row_base, int max_c4,
                         uint64_t seed, int t_local, int t_total, int t_first, int t_stride, hipStream_t s);

// ---------------------------------------------------------------- post-process (kernels_post.hip, NMS: kernels_nms.hip)
struct LevelTable {
  int num_levels;
  int hw[UDA_MAX_LEVELS];
  int a_off[UDA_MAX_LEVELS + 1];   // anchor offset of each level; a_off[num_levels] = A_tot
  const float* cls[UDA_MAX_LEVELS]; // [n*Tc, hw, A*C]
  const float* box[UDA_MAX_LEVELS]; // [n*Tb, hw, boxch]
};

struct AggArgs {
  LevelTable lv;
  const float* anchors;  // [A_tot, 4]
  int n_img, A_tot, A, C;
  int K;                 // candidates per image: A_tot (argmax path) or max_nms_inputs (top-k path)
  const int32_t* cand_flat;  // [n, K] flat (anchor*C + class) indices of the top-k path, or null
  int Tc, Tb;            // samples carried by the class / box head outputs (1 = not stacked)
  int loss_att;
  int decode;            // uda_decode
  float* boxes;          // [n, A_tot, 4]
  float* scores;         // [n, A_tot]
  int32_t* classes;      // [n, A_tot]
  float* logits;         // [n, A_tot, C]  mean logits
  float* u_cls;          // [n, K, C] (argmax path) / [n, K, 1] (top-k path) or null
  float* u_al;           // [n, A_tot, 4] or null
  float* u_ep;           // [n, A_tot, 4] or null
  int park_all, cls_slots;   // set by launch_aggregate: LDS parking layout of the class logits
  int decode_nsamples;       // UDA_DECODE_SAMPLE: draws per (candidate, MC sample)
  uint64_t decode_seed;      //   seed of the Philox normal stream
  uint32_t row_base;         //   global sample-row index of image 0 of this range: (image offset + i0) * Tb
};
void launch_aggregate(const AggArgs& a, hipStream_t s);
// mean logits of every (anchor, class): out [n, A_tot*C]   (input of the top-k pre-selection)
void launch_class_mean(const AggArgs& a, float* out, hipStream_t s);
// per image: the k largest of vals[n][0..L) -> flat indices, value descending, ties -> lower index
// ws: scratch of topk_workspace_bytes(n_img, k) bytes for the multi-block selection (null: one block per image)
void launch_topk(const float* vals, int n_img, int L, int k, int32_t* out_idx, void* ws, hipStream_t s);
size_t topk_workspace_bytes(int n_img, int k);

struct PreGeo {          // one raw image of a batch (raw sizes may differ between images: KITTI has four)
  unsigned long long off;     // byte offset of the image in the packed uint8 buffer
  int h, w;                   // raw size
  int sh, sw;                 // scaled size inside the H x W network input (the rest is zero padding)
  float scale_y, scale_x;     // raw / scaled ratios of the bilinear sampler
  float inv_scale;            // image_scale handed to the post-process
  int pad_;
};
struct PreprocArgs {
  const uint8_t* in;   // images back to back, image i = [geo[i].h, geo[i].w, 3] at geo[i].off
  float* out;          // [n, H, W, 3]
  const PreGeo* geo;   // [n] (device)
  int n, H, W;
  float mean[3], stdv[3];
  int noise;           // 1: the consistency check's noise variant (raw + sqrt(0.5) N(0, 1) in float64, kernels_post.hip raw_px)
  uint64_t noise_seed; //   Philox key of the draws (the run's dropout seed)
  uint32_t noise_img0; //   image index of image 0 in the counter (the dropout image offset)
};
void launch_preprocess(const PreprocArgs& a, hipStream_t s);

// consistency check (reference infer_model.py:768-848): flip and blur of n staged uint8 images, written behind them
struct AugArgs {
  uint8_t* img;                     // packed raw images (image i at img + geo[i].off); flips at + variant_stride, blurs at + 2 variant_stride
  const PreGeo* geo;                // [n] (device)
  unsigned long long variant_stride;  // bytes of the n originals
  int n;
};
void launch_augment_u8(const AugArgs& a, int max_h, int max_w, hipStream_t s);
struct ConsArgs {
  const float* boxes;    // [4n, M, bc] detections: originals, then the flip, blur and noise variants
  const float* classes;  // [4n, M, cc] (column 0: class id)
  const PreGeo* geo;     // [n] raw sizes of the originals (the flip is undone with the raw width)
  double* iou;           // [n, M] cons_iou
  uint8_t* agree;        // [n, M] cons_cls
  int n, M, bc, cc;
};
void launch_consistency(const ConsArgs& a, hipStream_t s);

// ground-truth assignment (reference utils_extra.py:44-64; validate_model.py:314-339, calibrate_model.py:133-147)
enum { ASSIGN_IOU = 0, ASSIGN_MSE = 1, ASSIGN_RANK = 2 };
enum { ASSIGN_KEEP_VALIDATE = 0, ASSIGN_KEEP_CALIBRATE = 1 };
struct AssignArgs {
  const float* det_boxes;   // [n, M, det_stride] y1 x1 y2 x2 in the first four columns
  const float* gt_boxes;    // [n, G, 4]
  const float* gt_classes;  // [n, G] (-1 rows: padding)
  int32_t* det_index;       // [n, G] matched rank, -1 = row not kept
  double* iou;              // [n, G] calc_iou_np(gt, matched box), 0 = row not kept
  int32_t* count;           // [n] kept rows
  int32_t* err;             // set to 1 when the rank method meets a kept row >= M
  int n, M, G, det_stride, method, keep;
};
void launch_assign_gt(const AssignArgs& a, hipStream_t s);
struct AssignRowsArgs {
  const int32_t* det_index; // [n, G]
  const int32_t* count;     // [n]
  const float *boxes, *scores, *classes, *logits, *probs, *entropy;   // the detection outputs (logits / probs / entropy: C > 0)
  float* rows;              // [sum(count), cols]
  int n, M, G, bc, cc, C, cols;   // cols = bc + 1 + cc + (C ? 2 C + 1 : 0)
};
void launch_gather_assigned(const AssignRowsArgs& a, hipStream_t s);

// active-learning image scores (reference active_learning_loop.py:528-765): T = float for the columns resident in a handle,
// double for host arrays (uda_score_images_np)
template <typename T>
struct ScoreArgs {
  const T* boxes;           // [n, M, box_stride] y1 x1 y2 x2 in the first four columns
  const T* scores;          // [n, M]
  const T* classes;         // [n, M, cls_stride] class id 1..C in the first column
  const T* entropy;         // [n, M] (source ENTROPY)
  const T *albox, *mcbox;   // first of the 4 std columns of row 0, rows al_stride / mc_stride apart
  const T* mcclass;         // first of the mcc_w std columns of row 0, rows mcc_stride apart
  double* comp;             // [n, n_comp]
  int32_t* count;           // [n] kept rows
  int32_t* class_counts;    // [n, C] kept rows per class id 1..C
  int32_t* err;             // set to 1 by a kept row whose class id is not one of 1..C
  int n, M, C, box_stride, cls_stride, al_stride, mc_stride, mcc_stride, mcc_w;
  T min_score;              // a row is kept iff score > min_score
  uda_score_desc_t desc;
};
void launch_score_images(const ScoreArgs<float>& a, hipStream_t s);
void launch_score_images(const ScoreArgs<double>& a, hipStream_t s);

// pseudo-labelling rows (reference SSL_stac.py:302-642, STAC.score_image): the per-ROW form of the scores above.  `s` gives the
// columns, min_score and the descriptor (its comp / count / class_counts / reduce_mean are not used); one record per candidate row
struct PseudoRecord {       // uda_pseudo_record_t
  int32_t image, row;
  float box[4];             // as stored: y1 x1 y2 x2
  float det_score;
  int32_t cls;
  double v;
};
static_assert(sizeof(PseudoRecord) == 40, "the record is 40 bytes");
template <typename T>
struct PseudoArgs {
  ScoreArgs<T> s;
  double tau;               // a candidate: det_score > tau (gate 0) or v > tau (gate 1), in float64
  int invert, gate;         // invert: v = 1 / mean of the 2 or 3 components; else v = the one component
  int max_rows, cap;        // only the first max_rows kept rows of an image take part; cap = min(M, max_rows) slots per image
  double* minmax;           // [n, 2] over the participating rows, NaN ignored; (+inf, -inf) where none takes part
  int32_t *kept, *cand;     // [n] rows above min_score (before the cap) / candidates
  PseudoRecord* slots;      // [n, cap] the image's candidates in rank order (staging for the packing kernel)
  PseudoRecord* records;    // [sum(cand)] densely packed in (image, rank) order
};
void launch_pseudo_rows(const PseudoArgs<float>& a, hipStream_t s);
void launch_pseudo_rows(const PseudoArgs<double>& a, hipStream_t s);

// COCO matching (reference custom_cocoeval.py:265-349 on the containers of coco_metric.py:219-283): one record per detection row
enum { COCO_MAX_DET = 100, COCO_MAX_M = 4096, COCO_MAX_G = UDA_EVAL_MAX_GT, COCO_MAX_T = UDA_EVAL_MAX_THRS };
struct CocoMatchArgs {
  const float* rows;        // legacy layout: [n, M, 7] image id, x, y, w, h, score, class
  const float* boxes;       // resident layout: [n, M, box_stride] y1 x1 y2 x2 in the first four columns
  const float* scores;      //                  [n, M]
  const float* classes;     //                  [n, M, cls_stride] class id in the first column
  const float* gt;          // [n, G, 7] y1, x1, y2, x2, is_crowd, area (not read), class; class <= -1: padding row
  uda_eval_record_t* rec;   // [n, M]
  int32_t* npig;            // [n, C, 4] non-ignored ground-truth rows per class id 1..C and area range
  int32_t* used;            // [n] rows with class > -1
  int n, M, G, C, T, box_stride, cls_stride, legacy;
  double thr[COCO_MAX_T];
};
void launch_coco_match(const CocoMatchArgs& a, hipStream_t s);

// thresholding: the batched ROC objective (reference uncertainty_analysis.py:44-152 on sklearn's roc_curve).  One chunk of Pc
// candidates per launch_thr_objective: combined score -> (descending key, row) sorted per candidate -> one curve per (candidate,
// IoU threshold).  Every buffer is the caller's; launch_thr_mask fills `mask` once per call.
enum { THR_MAX_N = UDA_THR_MAX_N, THR_MAX_U = UDA_THR_MAX_U, THR_MAX_K = UDA_THR_MAX_THRS, THR_MAX_P = UDA_THR_MAX_P,
       THR_MAX_G = UDA_THR_MAX_G, THR_TILE = 2048, THR_MAX_CHUNK = 16384 };
struct ThrArgs {
  const double* uncerts;    // [U, N]; row j starts at uncerts + j * ld
  const double* ious;       // [N]
  const uint8_t* tp_class;  // [N]
  const int32_t* group;     // [N] values 0..G-1, or null (G = 0)
  const double* params;     // [Pc, U * max(G, 1)]
  uint32_t* mask;           // [N] bit k: (ious >= thr[k]) && tp_class
  uint64_t* keys;           // [Pc, Npad] scratch: ~(order-preserving bits of the combined score), padded with ~0
  int32_t* rows;            // [Pc, Npad] scratch: the row a key came from
  int32_t* runs;            // [Pc, K, 2, N] scratch: last sorted position of every run of equal scores, positives up to it
  double* out;              // [Pc, K, 3] thr, rate, auc
  int N, Npad, U, G, K, Pc, fix_cd;
  int ld;                   // row stride of uncerts, 0: N.  A caller that works on rows [lo, lo + N) of a wider table passes the
                            // pointers moved by lo and the table's width here (uda_thr_report_np)
  double budget;
  double thr[THR_MAX_K];
};
void launch_thr_mask(const ThrArgs& a, hipStream_t s);
void launch_thr_objective(const ThrArgs& a, hipStream_t s);

// thresholding report (kernels_thrrep.hip): what the reference computes next to the curve of one (segment, score column, IoU
// threshold) - label counts, the moments behind calc_jsd, the removal counts at the threshold the curve gave.  One block each.
enum { THRREP_MAX_S = UDA_THR_REPORT_MAX_S, THRREP_MAX_B = UDA_THR_REPORT_MAX_SEGS, THRREP_ROWS = 256, THRREP_UNROLL = 8 };
struct ThrRepArgs {
  const double* scores;     // [S, N]
  const uint32_t* mask;     // [N] of launch_thr_mask
  const int32_t* seg_lo;    // [B]
  const int32_t* seg_hi;    // [B]
  double* roc;              // [B, S, K, 3] thr, rate, auc: filled by launch_thr_report_fill, then by the curves, read for thr
  long long* n_label;       // [B, K, 2] rows with correct, rows without
  double* moments;          // [B, S, K, 2, 2] (correct | wrong) x (sum, m2)
  long long* removed;       // [B, S, K, 3] correctly removed, falsely removed, falsely remaining
  int N, S, K, B;
};
void launch_thr_report_fill(const ThrRepArgs& a, hipStream_t s);
void launch_thr_report(const ThrRepArgs& a, hipStream_t s);

// post-thresholding analysis (kernels_thrpost.hip): M heat maps of H x W from row rectangles in one launch, one block per (tile, map),
// and the tallies behind the spider metrics and the image ranking, one block per IoU threshold
enum { HEAT_TILE_H = UDA_HEAT_TILE_H, HEAT_TILE_W = UDA_HEAT_TILE_W, HEAT_CHUNK = UDA_HEAT_CHUNK, HEAT_MAX_M = UDA_HEAT_MAX_MAPS,
       HEAT_MAX_R = UDA_HEAT_MAX_RECTS, HEAT_MAX_V = UDA_HEAT_MAX_VALUES, HEAT_MAX_Q = UDA_HEAT_MAX_SELS,
       HEAT_MAX_PIXELS = UDA_HEAT_MAX_PIXELS };
struct HeatArgs {
  const int4* rects;        // [R, N] r0, r1, c0, c1: half-open ranges inside the map (validated on the host)
  const double* values;     // [V, N]
  const uint8_t* sel;       // [Q, N]
  double* heat;             // [M, H, W]
  int32_t* count;           // [M, H, W] or null
  int N, H, W, tiles_x;
  int map_rect[HEAT_MAX_M], map_value[HEAT_MAX_M], map_sel[HEAT_MAX_M], map_mean[HEAT_MAX_M];
};
void launch_heat_maps(const HeatArgs& a, int tiles, int M, hipStream_t s);
enum { THRPOST_ROWS = 256, THRPOST_UNROLL = 4 };
struct ThrPostArgs {
  const double* u;          // [N]
  const double* ious;       // [N]
  const uint8_t* tp;        // [N]
  const int32_t* image;     // [N] ids 0..I-1 (validated on the host); read by the block of k_img only
  long long* counts;        // [K, 2, 4] removed | remaining: rows, tp_class rows, correct, wrong
  double* iou_sum;          // [K, 2]
  int32_t* img_count;       // [I, 4], zeroed
  int32_t* img_first;       // [I, 3], filled with N
  int N, K, k_img;          // k_img < 0: no per-image outputs
  double iou_thr[THR_MAX_K], thr[THR_MAX_K];
};
void launch_thr_post(const ThrPostArgs& a, hipStream_t s);

// dataset pruning: the neighbour rows of extract_hash_matrix (reference active_learning_loop.py:240-270) as four passes with a
// launch boundary between them: max -> (host: limit) -> count -> scan -> (host: total, idx allocated) -> fill.  A block is
// PRUNE_ROWS rows and walks the chunks_per_span chunks of PRUNE_COLS columns of its span (grid.y = spans); a slot is one
// (row, span), in that order.  Every buffer is the caller's.
enum { PRUNE_ROWS = UDA_PRUNE_ROWS, PRUNE_COLS = UDA_PRUNE_COLS, PRUNE_MAX_W = 4, PRUNE_SCAN_TILE = 2048, PRUNE_SCAN_MAX_TILES = 1024 };
struct PruneArgs {
  const uint64_t* hashes;   // [N, W]
  int32_t* max_dist;        // [1], zeroed by the caller
  int32_t* counts;          // [n_slots] columns within the limit
  int64_t* tile_sums;       // [n_tiles + 1] scratch of the scan; the total ends up behind the tiles
  int64_t* cursor;          // [n_slots] first entry of the slot in idx
  int64_t* row_off;         // [N + 1]
  int32_t* idx;             // [total]
  int N, W, n_chunks, spans, chunks_per_span, n_tiles;
  int64_t n_slots;          // N * spans
  double limit;             // a column is a neighbour iff (double)d <= limit
};
void launch_prune_max(const PruneArgs& a, hipStream_t s);
void launch_prune_count(const PruneArgs& a, hipStream_t s);
void launch_prune_scan(const PruneArgs& a, hipStream_t s);
void launch_prune_fill(const PruneArgs& a, hipStream_t s);

// set similarity: the nearest-neighbour squared distances of emp_KL_divergence (reference active_learning_eval.py:481-487) for B
// ragged problems in one launch (kernels_knn.hip).  The host cuts every problem into work items: KNN_ROWS queries x the chunks
// [c0, c1) of KNN_COLS reference points; items of one row block that cover different spans meet in d2_bits by atomicMin.
enum { KNN_ROWS = UDA_KNN_ROWS, KNN_COLS = UDA_KNN_COLS, KNN_MAX_D = UDA_KNN_MAX_D, KNN_MAX_ITEMS = 1 << 23 };
struct KnnItem {
  int32_t problem, row0, c0, c1;   // queries [row0, row0 + KNN_ROWS) of the problem against its reference chunks [c0, c1)
};
struct KnnArgs {
  const double* queries;    // [q_off[B], D]
  const double* refs;       // [r_off[B], D]
  const int64_t* q_off;     // [B + 1]
  const int64_t* r_off;     // [B + 1]
  const uint8_t* self;      // [B] reference row j is the query row j itself and is left out; null: no problem is one
  const KnnItem* items;     // [n_items]
  unsigned long long* d2_bits;   // [total] the bit patterns of the minima; filled with +inf by the launch itself
  int64_t total;            // q_off[B]
  int D, n_items;
};
void launch_knn_min(const KnnArgs& a, hipStream_t s);

// Gaussian KDE evaluation (reference uncertainty_ep_vs_al.py:361-375: gaussian_kde on a mesh) for B ragged problems
// (kernels_kde.hip).  The host cuts every problem into work items: KDE_POINTS points x the runs [r0, r1) of KDE_RUN data rows; an
// item writes the sequential sum of each of its runs to run_sums, and a second launch folds a point's run sums in the stated tree.
// The cut into items decides who sums a run and nothing about any value.
enum { KDE_POINTS = UDA_KDE_POINTS, KDE_RUN = UDA_KDE_RUN, KDE_MAX_D = UDA_KDE_MAX_D, KDE_MAX_ITEMS = 1 << 22 };
struct KdeItem {
  int32_t problem, point0, r0, r1;   // points [point0, point0 + KDE_POINTS) of the problem against its runs [r0, r1)
};
struct KdeTile {
  int32_t problem, point0;           // the tree launch: points [point0, point0 + KDE_POINTS) of the problem
};
struct KdeArgs {
  const double* data;       // [d_off[B], D] whitened rows
  const double* weight;     // [d_off[B]]; null: every row counts 1 and is not multiplied
  const double* points;     // [p_off[B], D] whitened points
  const int64_t* d_off;     // [B + 1]
  const int64_t* p_off;     // [B + 1]
  const int64_t* s_off;     // [B + 1] where the problem's run sums [runs_b, m_b] begin in run_sums
  const KdeItem* items;     // [n_items]
  const KdeTile* tiles;     // [n_tiles]
  double* run_sums;         // [s_off[B]]; every element is written by exactly one item before the tree launch reads it
  double* sum;              // [p_off[B]]
  int D, n_items, n_tiles;
};
void launch_kde_eval(const KdeArgs& a, hipStream_t s);

// label correction (reference ssl_utils/glc.py): the three verdicts on one image's kept detections and counted ground-truth rows
// (kernels_glc.hip).  T = float for the columns resident in a handle, double for host arrays (uda_label_check_np)
enum { LC_MD = UDA_LC_MD, LC_MISTAKES = UDA_LC_MISTAKES, LC_NOISY = UDA_LC_NOISY };
enum { LC_MD_EQ = UDA_LC_MD_EQ, LC_MD_LE = UDA_LC_MD_LE };
enum { LC_GT_MISTAKE = UDA_LC_GT_MISTAKE, LC_GT_NOISY = UDA_LC_GT_NOISY, LC_GT_REPLACED = UDA_LC_GT_REPLACED };
enum { LC_DET_KEPT = UDA_LC_DET_KEPT, LC_DET_MISSING = UDA_LC_DET_MISSING };
template <typename T>
struct LabelCheckArgs {
  const T* det_boxes;       // [n, M, det_stride] y1 x1 y2 x2 in the first four columns
  const T* scores;          // [n, M]
  const double* cons_iou;   // [n, M]; null when neither md nor noisy is asked for
  const T* gt_boxes;        // [n, G, 4]
  const T* gt_classes;      // [n, G] a row counts iff class > 0 (-1 rows: padding)
  int32_t* det_rank;        // [n, G] rank of the matched detection, -1: row not counted / no kept detection
  double* iou;              // [n, G] the row's best IoU over the kept detections
  uint8_t* gt_flags;        // [n, G] LC_GT_*
  float* gt_boxes_out;      // [n, G, 4] the row's own box, or the detection's where replaced
  uint8_t* det_flags;       // [n, M] LC_DET_*
  double* det_max_iou;      // [n, M] the detection's best IoU over the counted rows (0: not kept)
  int32_t* counts;          // [n, 5] kept detections, counted rows, mistakes, replaced rows, missing labels
  int32_t* first_row;       // [n, M] scratch: first row matched to a packed detection
  int n, M, G, det_stride, methods, md_rule;
  T min_score, correct_score;   // kept: score > min_score; noisy: score >= correct_score - in the scores' own type
  double iou_consist, md_max_inter, correct_max_inter;
};
void launch_label_check(const LabelCheckArgs<float>& a, hipStream_t s);
void launch_label_check(const LabelCheckArgs<double>& a, hipStream_t s);

// pseudo-label audit (reference ssl_utils/parent.py:1567-1813): B ragged images, one block each (kernels_audit.hip).  Every output
// is a device buffer of the call's own; rows and labels are addressed by the offsets, indices are within the image.
struct AuditArgs {
  const double* gt_boxes;       // [gt_off[B], 4]
  const double* det_boxes;      // [det_off[B], 4]
  const int64_t* gt_off;        // [B + 1]
  const int64_t* det_off;       // [B + 1]
  double* gt_max_iou;           // per row: the best IoU over the image's labels
  int32_t* gt_best_det;         //          the first label that reaches it
  int32_t* gt_alloc_det;        //          the matched prediction that took the row, -1: none
  uint8_t* gt_flags;            //          UDA_AUDIT_GT_*
  double* det_max_iou;          // per label: the best IoU over the image's rows
  int32_t* det_best_gt;         //            the first row that reaches it
  int32_t* det_alloc_gt;        //            the row a matched prediction took, -1: not a matched prediction
  double* det_alloc_miou;       //            np.max of that row in the reference's mutated matrix
  double* det_alloc_pair_iou;   //            IoU of the allocated pair, 0 where not allocated
  uint8_t* det_flags;           //            UDA_AUDIT_DET_*
  int32_t* n_matches;           // [B] matched predictions of the image
  int B, max_g, max_d;          // max_g / max_d: the call's largest image, they size the block's LDS
  double gt_iou_thr;
};
void launch_pseudo_audit(const AuditArgs& a, hipStream_t s);

// validation uncertainty report (reference utils_extra.py:378-445, calibrate_regression.py:231-349, utils_box.py:17-102): B ragged
// segments of matched rows x K sigma columns (kernels_report.hip).  The host cuts every segment into runs of REPORT_ROWS rows counted
// from the segment's start; a block takes one (run, column).  Counters meet by integer atomics; a float64 sum is the root of the
// zero-padded pairwise tree over the segment's rows: the block leaves the root of its run in `partials`, the second kernel folds
// the segment's runs (padded to a power of two, slots pbase[b] .. pbase[b + 1]) in place.
enum { REPORT_ROWS = UDA_REPORT_ROWS, REPORT_MAX_L = UDA_REPORT_MAX_L, REPORT_SEG_SUMS = 2, REPORT_COL_SUMS = 3 };
struct ReportItem {
  int32_t seg, row0, slot;      // rows [row0, row0 + REPORT_ROWS) of the segment; slot: where its partial sums go
};
struct ReportArgs {
  const double* gt;             // [rows, 4]
  const double* pred;           // [rows, 4]
  const double* gt_class;       // [rows]
  const double* cls;            // [rows]
  const double* sigma;          // [K, rows, 4]
  const double* z;              // [L]
  const int64_t* off;           // [B + 1]
  const int64_t* pbase;         // [B + 1] first partial slot of a segment; a segment holds a power of two of them, or none
  const ReportItem* items;      // [n_items]
  unsigned long long* seg_counts;   // [B, 4]      n_rows (the host's) | n_iou_zero | n_misclassified | n_gt_nonzero
  unsigned long long* col_counts;   // [B, K, 3]   covered_all | n_res_nonzero | n_degenerate
  unsigned long long* ece_count;    // [B, K, 4, L]
  double* seg_sums;             // [B, 2]      S_iou | S_sqerr
  double* col_sums;             // [B, K, 3]   S_sigma2 | S_ue | S_nll
  double* partials;             // [2 + 3 K, slots], zeroed
  int64_t rows, slots;
  int B, K, L, n_items;
};
void launch_uncert_report(const ReportArgs& a, hipStream_t s);

// classification calibration report (reference calibrate_classification.py:97-143, 250-440): B ragged segments of rows x M probability
// tables x (C + 1) targets (kernels_classrep.hip).  The host cuts every segment into runs of CLASSREP_ROWS rows counted from the
// segment's start; a block takes one (run, table) and walks the targets.  Counters meet by integer atomics; a float64 sum is the root
// of the zero-padded pairwise tree over the segment's rows: the block of a segment of ONE run writes the output itself (slot < 0), a
// block of a longer segment leaves the root of its run in `partials` and the second kernel folds the segment's runs (padded to a
// power of two, slots pbase[b] .. pbase[b + 1]; none for a segment of at most one run) in place.
enum { CLASSREP_ROWS = UDA_CLASSREP_ROWS, CLASSREP_MAX_E = UDA_CLASSREP_MAX_E };
struct ClassRepItem {
  int32_t seg, row0, slot;      // rows [row0, row0 + CLASSREP_ROWS) of the segment; slot: where its partial sums go, -1: to the outputs
};
struct ClassRepArgs {
  const double* prob;           // [M, rows, C]
  const int32_t* label;         // [rows]
  const double* edges;          // [G, E]
  const int32_t* n_edges;       // [G]
  const int64_t* off;           // [B + 1]
  const int64_t* pbase;         // [B + 1] first partial slot of a segment
  const int32_t* tree_segs;     // [n_tree] the segments of more than one run
  const ClassRepItem* items;    // [n_items]
  unsigned long long* bin_count;    // [B, M, C + 1, E + 1]
  unsigned long long* bin_hits;     // [B, M, C + 1, E + 1]
  unsigned long long* tab_counts;   // [B, M, 2]   rows whose q was clipped | rows left out of the NLL
  double* bin_sum;              // [B, M, C + 1, E + 1]
  double* brier_sum;            // [B, M, C]
  double* nll_sum;              // [B, M]
  double* partials;             // [M * ((C + 1) * (E + 1) + C + 1), slots], zeroed
  int64_t rows, slots;
  int B, M, C, G, E, n_items, n_tree;
};
void launch_class_report(const ClassRepArgs& a, hipStream_t s);

// RCC collages (reference ssl_utils/parent.py:317-686): Pillow's two-pass 8-bit Lanczos resample, many jobs per call
// (kernels_collage.hip).  A job is one or two passes; a pass resamples one axis of a packed RGB plane with a table of
// resample_coeffs.  Every address is a byte offset into the call's one device allocation.
enum { RESAMPLE_THREADS = 256, RESAMPLE_TW = UDA_RESAMPLE_TILE, RESAMPLE_KCH = 16, RESAMPLE_SPAN_PER_POS = 32, RESAMPLE_LDS = 24576,
       RESAMPLE_BITS = 22 };
struct ResamplePass {
  int64_t src, dst;             // first byte of the source plane / of the pass's rectangle in the destination
  int64_t src_stride, dst_stride;   // bytes a row
  int64_t coef_off;             // into the int32 pool: bounds [out_full, 2], then coefficients [out_full, ksize]
  int32_t in_size, out_full;    // the axis: source length, and the length of the table (the unclipped output)
  int32_t n_out, n_lines;       // what is written: output positions along the axis (clipped), lines across it (clipped)
  int32_t ksize, tw;            // tw: output positions a tile, a power of two; a tile has RESAMPLE_THREADS / tw lines
  int32_t tile0, tiles_pos;     // first block of the pass in its launch; tiles along the axis
};
void launch_resample_passes(const ResamplePass* passes, int n_pass, int n_tiles, bool vertical, const int32_t* pool, uint8_t* base,
                            hipStream_t s);
int resample_ksize(int in_size, int out_size, int filter);    // filter: UDA_FILTER_LANCZOS | UDA_FILTER_BICUBIC
void resample_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk);

// The perceptual hash after its first resize (kernels_phash.hip): one block an image on the image's 512 x 256 RGB plane - grey,
// Lanczos to 32 x 32, the 8 x 8 corner of the DCT in float64, median, bits.  The tables are the call's, built on the host.
enum { PHASH_THREADS = 256, PHASH_WAVES = PHASH_THREADS / 64, PHASH_W = UDA_PHASH_PRE_W, PHASH_H = UDA_PHASH_PRE_H,
       PHASH_SIDE = UDA_PHASH_SIDE, PHASH_LOW = UDA_PHASH_LOW, PHASH_KX = 97, PHASH_KY = 49 };
struct PhashTables {
  double T[PHASH_LOW * PHASH_SIDE];                    // T[k][i] = 2 cos(pi k (2 i + 1) / 64)
  int32_t bx[2 * PHASH_SIDE], by[2 * PHASH_SIDE];      // (xmin, xmax) of resample_coeffs(512, 32) and (256, 32), Lanczos
  int32_t kx[PHASH_SIDE * PHASH_KX], ky[PHASH_SIDE * PHASH_KY];
};
void phash_dct_table(double* T);
void launch_phash_tail(const uint8_t* pre, int n, const PhashTables* tab, unsigned long long* words, double* margin, uint8_t* thumb,
                       double* low, hipStream_t s);

// RCC's manual augmentations (reference ssl_utils/parent.py:261-315) between a collage's resizes and pastes: kernels_augment.hip.
// Every address is a byte offset into the call's one device allocation, as for the resample passes.
enum { AUG_THREADS = 256, AUG_TILE = UDA_AUGMENT_TILE, AUG_ROWS = AUG_THREADS / AUG_TILE, AUG_MEAN_PIX = 16 * AUG_THREADS,
       BLUR_LINES = UDA_AUGMENT_TILE, BLUR_HALO = 3 * (UDA_BLUR_MAX_BOX + 1), BLUR_EXT = AUG_TILE + 2 * BLUR_HALO,
       BLUR_LDS = 2 * BLUR_LINES * 3 * BLUR_EXT };
enum { AUG_COPY = 0, AUG_FLIP = 1, AUG_BLEND = 2, AUG_BLEND_CLIP = 3, AUG_ADD = 4 };
struct AugJob {                 // one pointwise job: flip, blend, add bytes (and the copy a blur of radius 0 is)
  int64_t src, dst;             // first byte of the source plane / of the job's rectangle in the destination
  int64_t src_stride, dst_stride;
  int64_t noise;                // AUG_ADD: first byte of the job's noise in the call's noise array
  int64_t n_pix;                // pixels of the source plane (the contrast mean's divisor)
  int32_t w, cw, ch;            // the source's width; what is written (clipped)
  int32_t kind;
  float a;                      // AUG_BLEND*: f32(factor)
  int32_t mean;                 // AUG_BLEND*: slot of the plane's luma sum (contrast), -1: the degenerate is black (brightness)
  int32_t tile0, tiles_x;       // first block of the job in its launch; tiles along x
};
struct AugMeanJob {             // the luma sum of one contrast job's source plane
  int64_t src, n_pix;
  int32_t slot, tile0;
};
struct BlurPass {               // one stage (three box passes along one axis) of one blur job
  int64_t src, dst, src_stride, dst_stride;
  uint32_t ww, fw;
  int32_t r;                    // int(fr)
  int32_t n;                    // the line's true length
  int32_t n_out, n_lines;       // what is written: positions 0 .. n_out - 1 (clipped), lines across (clipped)
  int32_t tile0, tiles_pos;
};
void launch_augment_means(const AugMeanJob* jobs, int n_jobs, int n_tiles, unsigned long long* sums, const uint8_t* base, hipStream_t s);
void launch_augment_points(const AugJob* jobs, int n_jobs, int n_tiles, const unsigned long long* sums, const uint8_t* noise, uint8_t* base,
                           hipStream_t s);
void launch_blur_stages(const BlurPass* passes, int n_pass, int n_tiles, bool vertical, uint8_t* base, hipStream_t s);
void gauss_box(double radius, float* fr, uint32_t* ww, uint32_t* fw);

struct NmsArgs {
  const float* boxes;    // [n, K, 4]
  float* stale;          // [n, K]  working scores (dead = -inf)
  int32_t* begin;        // [n, K]
  float* tent;           // [n, K]  updated score computed in epoch ev[i]
  float* ub;             // [n, K]  upper bound of the candidate's updated score in every later epoch
  int32_t* ev;           // [n, K]  epoch of the last evaluation (-1 = never)
  int32_t* sel_idx;      // [n, M]
  float* sel_score;      // [n, M]
  float* sel_box;        // [n, M, 4]
  unsigned long long* bound_key;  // [n, M]
  unsigned long long* win_key;    // [n, M]
  int32_t* nsel;         // [n]
  int32_t* done;         // [n]
  int n_img, K, M;       // n_img = number of NMS problems (images, or images*classes in per-class mode)
  float iou_thr, score_thr, scale;  // scale = soft ? -0.5/sigma : 0
  int soft;
  int segs;              // problems per image: 1 (global) or num_classes (per-class mode)
  const int32_t* classes;  // [images, K] candidate classes (per-class mode) or null
};
void launch_nms_init(const NmsArgs& a, const float* scores, hipStream_t s);
void launch_nms_epoch(const NmsArgs& a, int epoch, hipStream_t s);
// all epochs in one launch, one block per problem (kernels_nms.hip "NMS, one launch")
bool nms_solo_supported(const NmsArgs& a);
void launch_nms_solo(const NmsArgs& a, const float* scores, hipStream_t s);
// the same with the per-candidate state in registers, problems of up to 8192 candidates
bool nms_reg_supported(const NmsArgs& a);
void launch_nms_reg(const NmsArgs& a, const float* scores, hipStream_t s);

// all epochs of large problems in one launch of a co-resident grid; slots [n_img x nms_coop_slot_words(M)] / err [1] are scratch
size_t nms_coop_slot_words(int M);
int launch_nms_coop(const NmsArgs& a, const float* scores, unsigned long long* slots, int* err, hipStream_t s);   // 1 launched, 0 not its domain, -1 wanted but not launched

// NMS on the top-scoring prefix of a large candidate set (kernels_nms.hip "NMS on a score prefix")
struct PrefixArgs {
  const float* scores;   // [n, K]
  const float* boxes;    // [n, K, 4]
  int32_t* sub_idx;      // [n, Lcap]  candidate index of every prefix entry, ascending
  float* sub_scores;     // [n, Lcap]  (-inf padding)
  float* sub_boxes;      // [n, Lcap, 4]
  uint32_t* excl_key;    // [n]  order-preserving key of the largest excluded score (0 = nothing excluded)
  int32_t* bad;          // [n]  1 = the prefix cannot stand in for the full problem
  int n_img, K, Lp, Lcap;
};
void launch_prefix_select(const PrefixArgs& a, hipStream_t s);
struct PrefixCheckArgs {
  const int32_t* sub_sel_idx;   // [n, M] positions in the prefix
  const float* sub_sel_score;   // [n, M]
  const int32_t* sub_nsel;      // [n]
  const int32_t* sub_idx;       // [n, Lcap]
  const uint32_t* excl_key;     // [n]
  int32_t* sel_idx;             // [n, M] candidate indices (what the gather stage reads)
  float* sel_score;             // [n, M]
  int32_t* nsel;                // [n]
  int32_t* bad;                 // [n]
  int n_img, M, Lcap;
  float score_thr;
};
void launch_prefix_check(const PrefixCheckArgs& a, hipStream_t s);

struct GatherArgs {
  const int32_t* sel_idx;   // [n, M]
  const float* sel_score;   // [n, M]
  const int32_t* nsel;      // [n]
  const float* boxes;       // [n, K, 4]
  const int32_t* classes;   // [n, K]
  const float* logits;      // [n, K, C]
  const float* u_cls;       // or null
  const float* u_al;
  const float* u_ep;
  const float* scales;      // [n] image scales or null
  float* out_boxes;         // [n, M, box_cols]
  float* out_scores;        // [n, M]
  float* out_classes;       // [n, M, cls_cols]
  int32_t* out_valid;       // [n]
  float* out_logits;        // [n, M, C] or null
  int n_img, K, M, C, box_cols, cls_cols;
  int ucls_cols;            // class-std values per candidate: C (argmax path) or 1 (top-k path)
  float clip_h, clip_w;
  int clip;
};
void launch_gather(const GatherArgs& a, hipStream_t s);

struct MergeArgs {         // per-class mode: concat per-class selections, pad, top-M by score
  const int32_t* sel_idx;  // [images*C, M]
  const float* sel_score;  // [images*C, M]
  const int32_t* nsel;     // [images*C]
  const float* boxes;      // [images, K, 4]
  const float* scales;     // [images] or null
  unsigned long long* keys;  // workspace [images, C*M + M]
  float* out_boxes;        // [images, M, 4]
  float* out_scores;       // [images, M]
  float* out_classes;      // [images, M]
  int32_t* out_valid;      // [images]
  int n_img, K, M, C;
};
void launch_merge_per_class(const MergeArgs& a, hipStream_t s);
template <typename T>
struct NmsNpArgs {         // numpy NMS family (kernels_post.hip): problems = consecutive slices of dets
  const T* dets;           // [total, 5] x1 y1 x2 y2 score (sorted by score, descending, for hard / diou)
  const int32_t* off;      // [problems + 1]
  T* score;                // [total] workspace
  int32_t* state;          // [total] workspace
  T* out;                  // [total, 5] kept rows of each problem at its offset
  int32_t* n_out;          // [problems]
  int method;              // 0 hard, 1 diou, 2 gaussian, 3 linear
  T iou_thr, sigma, score_thr;
};
template <typename T>
void launch_nmsnp(const NmsNpArgs<T>& a, int n_problems, hipStream_t s);

struct CalibArgs {
  const float* boxes;     // [rows, box_cols] output boxes (+ uncertainty columns)
  const float* classes;   // [rows, cls_cols] class id in column 0
  float* out;             // [rows, 4]
  const double* xs;       // concatenated table thresholds
  const double* ys;
  const int32_t* tab_off; // [n_tables + 1]
  float temps[4];
  int rows, box_cols, cls_cols, col0;
  int mode, relative, n_tables;
};
void launch_calib(const CalibArgs& a, hipStream_t s);
void launch_probs(const float* logits, float* probs, float* entropy, int rows, int C, hipStream_t s);
struct PackDetArgs {
  const float *boxes, *scores, *classes, *logits;   // post-process outputs [n, M, bc] / [n, M] / [n, M, cc] / [n, M, C] (C = 0: no logits)
  const int32_t* valid;                             // [n]
  float* out;                                       // [rows_out, M, cols], cols = bc + 1 + cc + C + 1
  int n, rows_out, M, bc, cc, C, cols;
};
void launch_pack_det(const PackDetArgs& a, hipStream_t s);

struct ClsCalibArgs {
  const float* logits;    // [rows, C] mean logits of the selected rows
  const float* classes;   // [rows, cls_cols]: column 0 class id, columns 1..C the MC std of the logits (draws > 0)
  float* probs;           // [rows, C]
  float* entropy;         // [rows]
  float* uncert;          // [rows, C] std of the calibrated probabilities over the draws, or null
  const double* xs;       // isotonic tables (concatenated thresholds), 1 (all) or C (per class)
  const double* ys;
  const int32_t* tab_off; // [n_tables + 1]
  const float* temps;     // [C] temperature divisors (device)
  int rows, C, cls_cols;
  int mode;               // uda_class_calib_mode
  int draws;              // 0: calibrate the mean logits; > 0: that many normal draws per logit (the reference uses 10)
  uint64_t seed;
};
void launch_class_calib(const ClsCalibArgs& a, hipStream_t s);

}  // namespace uda
