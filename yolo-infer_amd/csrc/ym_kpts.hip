// Pose head: Ultralytics Pose.kpts_decode (non-export path) for the anchors NMS can emit.
//
// decode_anchors (ym_decode.hip) has appended, per image, one key per candidate (low 32 bits = ~anchor) and the
// candidate count.  This kernel runs behind it and before the NMS: for every candidate it reads the anchor's K·ndim
// raw keypoint values from the head rows and writes the decoded row
//   x = (raw·2 + gx)·stride, y = (raw·2 + gy)·stride, v = sigmoid(raw) (ndim 3), pad columns 0
// to a separate (B, A, nk_pad) buffer, which the NMS then reads its extras from (NmsArgs::anchors / mask_off / nm).
// raw·2 and ·stride (a power of two) are exact, so x and y round once and equal the fp32 CPU formula bit for bit
// (make_anchors' anchor − 0.5 is the integer grid index).  Rows of anchors that are no candidates keep whatever an
// earlier forward left there; the NMS reads candidates' rows only.
//
// Launch: the host does not know the counts, so the grid is fixed: KPT_CHUNKS workgroups per image, each
// grid-striding over min(counts[b], A) x nk_pad elements.  Consecutive lanes take consecutive columns of one
// candidate, so a candidate's raw row (204 bytes for COCO) is read contiguously and its decoded row written
// contiguously.  At conf 0.25 (tens of candidates per image) most workgroups take one pass or none.
#include "ym_common.h"

constexpr int KPT_T = 256;
constexpr int KPT_CHUNKS = 8;

__global__ __launch_bounds__(KPT_T) void kpts_decode(const KptArgs a) {
  const int b = blockIdx.x / KPT_CHUNKS, chunk = blockIdx.x - b * KPT_CHUNKS;
  int n = a.counts[b];
  if (n > a.A) n = a.A;
  const long total = (long)n * a.nk_pad;
  const int nk = a.K * a.ndim;
  const unsigned long long* keys = a.keys + (size_t)b * a.kstride;
  for (long i = (long)chunk * KPT_T + threadIdx.x; i < total; i += (long)KPT_CHUNKS * KPT_T) {
    const int cand = (int)(i / a.nk_pad);
    const int col = (int)(i - (long)cand * a.nk_pad);
    const unsigned anc = 0xFFFFFFFFu - (unsigned)(keys[cand] & 0xFFFFFFFFull);
    if (anc >= (unsigned)a.A) continue;  // not a key decode_anchors wrote
    const size_t row = (size_t)b * a.A + anc;
    float v = 0.f;
    if (col < nk) {
      const float raw = a.anchors[row * a.no_tot + a.kpt_off + col];
      const int d = col % a.ndim;
      if (d == 2) {
        v = ym_sigmoid(raw);
      } else {
        int l = 0;
        while (l + 1 < a.nl && (int)anc >= a.lvl_off[l + 1]) ++l;
        const int p = (int)anc - a.lvl_off[l];
        const int gy = p / a.lvl_W[l];
        const float g = (float)(d == 0 ? p - gy * a.lvl_W[l] : gy);
        v = __fmul_rn(__fadd_rn(__fmul_rn(raw, 2.0f), g), a.lvl_stride[l]);
      }
    }
    a.out[row * a.nk_pad + col] = v;
  }
}

hipError_t ym_launch_kpts(const KptArgs& a, hipStream_t st) {
  if (a.B < 1 || a.K < 1 || (a.ndim != 2 && a.ndim != 3) || a.K * a.ndim > a.nk_pad || a.kpt_off < 0 ||
      a.kpt_off + a.K * a.ndim > a.no_tot || a.nl < 1 || a.nl > 4 || a.kstride < a.A)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(kpts_decode, dim3(a.B * KPT_CHUNKS), dim3(KPT_T), 0, st, a);
  return hipGetLastError();
}
