// lt_mask.h — settings.json mask_eqn (rast_algebra's mask_eqn, utils.py:447-484) as a kernel
// generated per expression and compiled at run time with hiprtc. Included by lt_abi.hip (host
// code) after lt_index.h, whose code generator makes the straight-line body.
//
// The host (land_trendr_amd/index_eqn.py MaskProgram) turns the expression into a typed postfix
// program whose root is a boolean; an observation-pixel stays valid only where it is true:
//   valid[o*valid_stride + p] &= program(bands of obs o at pixel p)
// on the existing uint8 [K][Q] validity plane (a 0 is never turned into a 1). One streaming pass:
// the band planes the program names are read once, the validity bytes read once and written only
// where a thread clears one. Kernels per program:
//   lt_mask_kernel        one pixel per thread, any strides (also the head and tail of a row);
//   lt_mask_kernel_v<W>   W = 16, 8, 4 consecutive pixels per thread for unit pixel stride: one
//                         vector load per band (W elements) and one W-byte load / store of the
//                         validity bytes. The widest W in use keeps a band load at 16 bytes per
//                         lane (W = 16 / element size, at least 4): the width a coalesced
//                         streaming read runs at full rate with.
// The host entry point (lt_abi.hip lt_mask_apply) picks the widest W at which the band planes and
// the validity rows are both naturally aligned at some head offset < W, and sends the head and
// the tail to the scalar kernel.
// Every kernel walks its row in a grid-stride loop, the grid sized by the host entry point to a
// few blocks per CU in all (kTargetBlocks) whatever the row length.
// dropped (optional): the bytes turned from non-zero to 0, counted per thread over its loop,
// summed per wave with ballots once the loop is done, and added with one atomicAdd per wave. One
// atomicAdd per 8 x 64 pixels instead (a thread per vector, 2.9 M of them on the one counter at
// 7000 x 7000 x 30) made the pass 34.6 ms long; it takes 1.3 ms this way.
#pragma once
#include <hip/hiprtc.h>

#include <string>

struct lt_mask {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr, fnv[3] = {nullptr, nullptr, nullptr};  // scalar; W = 16, 8, 4
  int32_t n_bands = 0, band_type = 0;
};

namespace lt_msk {

constexpr int kWidths[3] = {16, 8, 4};

// the widest vector kernel a band type uses: 16-byte band loads (4 pixels at least)
inline int max_width(int band_type) {
  const int w = (int)(16 / lt_idx::type_size(band_type));
  return w < 4 ? 4 : w;
}

// blocks of 256 threads a launch aims at over all observations: 32 per CU of a 256-CU device
constexpr long long kTargetBlocks = 8192;

// the wave's sum of the threads' dropped counts added to *dropped by its first lane (every lane
// of the block reaches this, after its loop: no thread returns early): bit b of the counts is
// summed with one ballot, for as many bits as some lane has
constexpr const char* kCount = R"HIP(
__device__ static inline void lt_mask_count(unsigned long long* dropped, unsigned long long cnt) {
  if (!dropped) return;
  unsigned long long n = 0;
  for (int b = 0; b < 64 && __ballot((cnt >> b) != 0ull) != 0ull; b++)
    n += (unsigned long long)__popcll(__ballot((int)((cnt >> b) & 1ull))) << b;
  if (n != 0 && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(dropped, n);
}
)HIP";

// Generated source for the mask program P, or "" with err set.
inline std::string codegen(const lt_index_prog& P, std::string& err) {
  std::string root1, rootv;
  const std::string body1 = lt_idx::codegen_body(P, false, err, root1, true);
  if (body1.empty()) return "";
  const std::string bodyv = lt_idx::codegen_body(P, true, err, rootv, true);
  if (bodyv.empty()) return "";
  bool used[LT_MAX_BANDS] = {};
  for (int k = 0; k < P.n_ops; k++)
    if (P.ops[k].op == LT_OP_BAND) used[P.ops[k].ival] = true;  // (slots checked by codegen_body)
  const char* BT = lt_idx::ctype(P.band_type);
  std::string src = lt_idx::kPrelude;
  src += kCount;
  src += std::string("extern \"C\" __global__ __launch_bounds__(256) void lt_mask_kernel(const ") +
         BT + "* __restrict__ bands, long long obs_stride, long long band_stride, "
         "long long pix_stride, long long n_pix, unsigned char* __restrict__ valid, "
         "long long valid_stride, unsigned long long* dropped) {\n"
         "  const long long o = blockIdx.y;\n"
         "  unsigned long long cnt = 0;\n"
         "  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n_pix;\n"
         "       p += (long long)gridDim.x * 256) {\n"
         "  const " + BT + "* b = bands + o * obs_stride + p * pix_stride;\n";
  src += body1;
  src += "  unsigned char* vp = valid + o * valid_stride + p;\n"
         "  if (!" + root1 + " && *vp != 0) {\n    *vp = 0;\n    cnt++;\n  }\n"
         "  }\n  lt_mask_count(dropped, cnt);\n}\n";
  const int wmax = max_width(P.band_type);
  for (int w : kWidths) {
    const std::string W = std::to_string(w);
    if (w > wmax) continue;
    src += std::string("typedef ") + BT + " lt_bt" + W + " __attribute__((ext_vector_type(" + W +
           ")));\ntypedef unsigned char lt_vt" + W + " __attribute__((ext_vector_type(" + W +
           ")));\n";
    src += "extern \"C\" __global__ __launch_bounds__(256) void lt_mask_kernel_v" + W + "(const " +
           BT + "* __restrict__ bands, long long obs_stride, long long band_stride, "
           "long long n_pix, unsigned char* __restrict__ valid, long long valid_stride, "
           "unsigned long long* dropped) {\n"
           "  const long long o = blockIdx.y;\n"
           "  unsigned long long cnt = 0;\n"
           "  for (long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * " + W + "; p < n_pix;\n"
           "       p += (long long)gridDim.x * 256 * " + W + ") {\n"
           "  const " + BT + "* b = bands + o * obs_stride + p;\n";
    for (int s = 0; s < P.n_bands; s++)
      if (used[s])
        src += "  const lt_bt" + W + " bv" + std::to_string(s) + " = *(const lt_bt" + W +
               "*)(b + " + std::to_string(s) + "LL * band_stride);\n";
    src += "  lt_vt" + W + "* vp = (lt_vt" + W + "*)(valid + o * valid_stride + p);\n"
           "  lt_vt" + W + " vv = *vp;\n  unsigned drop = 0;\n#pragma unroll\n"
           "  for (int j = 0; j < " + W + "; j++) {\n";
    src += bodyv;
    src += "  if (!" + rootv + " && vv[j] != 0) {\n    vv[j] = 0;\n    drop++;\n  }\n"
           "  }\n  if (drop != 0) *vp = vv;\n  cnt += drop;\n"
           "  }\n  lt_mask_count(dropped, cnt);\n}\n";
  }
  return src;
}

}  // namespace lt_msk
