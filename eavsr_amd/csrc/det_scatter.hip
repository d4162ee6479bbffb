// The opt-in deterministic training mode (networks.set_deterministic): the input gradients of the training step's three
// scatter-shaped backward ops WITHOUT float atomics, each output element summed in an order that depends only on the inputs.
//
//   resize_bilinear_ac backward (backward.hip resize_ac_bwd_kernel: 4 float atomics per output pixel) -> a GATHER: every input pixel
//     finds the output pixels whose corners land on it analytically (a few candidate rows / columns around i / r), filters them with
//     exactly the forward's expressions (rw * ox, min((int)sx, win - 1), the edge rule) and adds their terms in increasing (oy, ox)
//     order.  No index, no workspace.
//   flow_warp backward dx (backward.hip flow_warp_bwd_kernel: 4 float atomics per pixel and channel) and DCNv2 dx (dcn_bwd.hip: global
//     atomics for corners outside the 13 x 32 LDS window) -> store-and-sum through an INVERTED INDEX per segment (a sample for flow_warp,
//     a (sample, deformable group) for DCNv2), built once and shared by every channel:
//       1. sample:  every source (pixel; (tap, pixel) for DCNv2) writes its four corner cells (-1: none) and corner weights, computed
//                   with the expressions of the atomic kernel;
//       2. count:   integer atomics count the entries per destination cell (a count does not depend on order);
//       3. scan:    exclusive prefix sum of the counts per segment (one workgroup per segment);
//       4. fill:    integer atomics deal each entry a slot in its cell's list (the slot order depends on timing ...);
//       5. rank:    ... so every entry counts the entries of its list with a smaller key (key = source * 4 + corner: unique) and is
//                   stored at that rank: each list ends up in ascending key order, whatever order the fill ran in;
//       6. gather:  one thread per (cell, channel) adds its list's contributions in that order.
//     The rank pass is quadratic in a list's length: a flow that collapses the image onto a few cells makes it slow, never wrong.
#include <algorithm>

#include "common.h"

namespace {

// ---- the index (steps 2-5).  Per segment: E entries (4 per source), ncell cells.  dst[s][E] (-1: no entry), off[s][ncell + 1],
// cur[s][ncell] (zeroed), list / sorted [s][E] (keys, in cell order from off[s][cell])
__global__ __launch_bounds__(256) void ds_zero_kernel(int* __restrict__ p, long count) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) p[i] = 0;
}

__global__ __launch_bounds__(256) void ds_count_kernel(const int* __restrict__ dst, int* __restrict__ off, int E, int ncell) {
  const int e = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (e >= E) return;
  const int d = dst[(size_t)s * E + e];
  if (d >= 0) atomicAdd(off + (size_t)s * (ncell + 1) + d, 1);
}

// counts -> exclusive offsets in place (off[ncell] = the segment's number of entries); one 1024-thread workgroup per segment
__global__ __launch_bounds__(1024) void ds_scan_kernel(int* __restrict__ off, int ncell) {
  __shared__ int s_sum[1024];
  int* o = off + (size_t)blockIdx.x * (ncell + 1);
  const int t = threadIdx.x;
  const int chunk = (ncell + 1023) / 1024;
  const int lo = min(t * chunk, ncell), hi = min(lo + chunk, ncell);
  int acc = 0;
  for (int i = lo; i < hi; ++i) acc += o[i];
  s_sum[t] = acc;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {      // inclusive Hillis-Steele scan of the per-thread sums
    const int v = t >= d ? s_sum[t - d] : 0;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  int run = s_sum[t] - acc;
  for (int i = lo; i < hi; ++i) {
    const int c = o[i];
    o[i] = run;
    run += c;
  }
  if (t == 1023) o[ncell] = s_sum[1023];
}

__global__ __launch_bounds__(256) void ds_fill_kernel(const int* __restrict__ dst, const int* __restrict__ off, int* __restrict__ cur,
                                                      int* __restrict__ list, int E, int ncell) {
  const int e = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (e >= E) return;
  const int d = dst[(size_t)s * E + e];
  if (d < 0) return;
  const int slot = atomicAdd(cur + (size_t)s * ncell + d, 1);
  const int pos = off[(size_t)s * (ncell + 1) + d] + slot;
  if (pos < off[(size_t)s * (ncell + 1) + d + 1]) list[(size_t)s * E + pos] = e;      // (always: the count pass counted it)
}

__global__ __launch_bounds__(256) void ds_rank_kernel(const int* __restrict__ dst, const int* __restrict__ off, const int* __restrict__ list,
                                                      int* __restrict__ sorted, int E, int ncell) {
  const int e = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (e >= E) return;
  const int d = dst[(size_t)s * E + e];
  if (d < 0) return;
  const int lo = off[(size_t)s * (ncell + 1) + d], hi = off[(size_t)s * (ncell + 1) + d + 1];
  const int* l = list + (size_t)s * E;
  int r = 0;
  for (int j = lo; j < hi; ++j) r += l[j] < e ? 1 : 0;
  if (lo + r < hi) sorted[(size_t)s * E + lo + r] = e;
}

// ---- step 1 for flow_warp: the sample position exactly as flow_warp_bwd_kernel computes it (flow2, the normalise / un-normalise
// pair, the +-4 clamp), its four corners and weights.  Source = pixel, segment = sample.
__global__ __launch_bounds__(256) void fw_det_sample_kernel(const float* __restrict__ flow, const float* __restrict__ flow2,
                                                            int* __restrict__ dst, float* __restrict__ wgt, int h, int w) {
  const int p = blockIdx.x * 256 + threadIdx.x, bn = blockIdx.y;
  const int plane = h * w;
  if (p >= plane) return;
  const int py = p / w, px = p - py * w;
  const size_t fo = (size_t)bn * 2 * plane + p;
  float fx = flow[fo], fy = flow[fo + plane];
  if (flow2) { fx += flow2[fo]; fy += flow2[fo + plane]; }
  const float gx = (float)px + fx, gy = (float)py + fy;
  const float nx = 2.0f * gx / (float)max(w - 1, 1) - 1.0f;
  const float ny = 2.0f * gy / (float)max(h - 1, 1) - 1.0f;
  float ix = ((nx + 1.0f) / 2.0f) * (float)(w - 1);
  float iy = ((ny + 1.0f) / 2.0f) * (float)(h - 1);
  ix = fminf(fmaxf(ix, -4.0f), (float)w + 4.0f);
  iy = fminf(fmaxf(iy, -4.0f), (float)h + 4.0f);
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
  const float wx1 = ix - fx0, wy1 = iy - fy0, wx0 = (fx0 + 1.0f) - ix, wy0 = (fy0 + 1.0f) - iy;
  const bool vx0 = (x0 >= 0) & (x0 < w), vx1 = (x1 >= 0) & (x1 < w);
  const bool vy0 = (y0 >= 0) & (y0 < h), vy1 = (y1 >= 0) & (y1 < h);
  const size_t e = ((size_t)bn * plane + p) * 4;
  dst[e + 0] = vx0 && vy0 ? y0 * w + x0 : -1;
  dst[e + 1] = vx1 && vy0 ? y0 * w + x1 : -1;
  dst[e + 2] = vx0 && vy1 ? y1 * w + x0 : -1;
  dst[e + 3] = vx1 && vy1 ? y1 * w + x1 : -1;
  wgt[e + 0] = wx0 * wy0;
  wgt[e + 1] = wx1 * wy0;
  wgt[e + 2] = wx0 * wy1;
  wgt[e + 3] = wx1 * wy1;
}

// ---- step 6 for flow_warp: dx[bn][c][cell] = sum over the cell's list, in key order, of dout[bn][c][pixel] * weight
__global__ __launch_bounds__(256) void fw_det_gather_kernel(const float* __restrict__ dout, const int* __restrict__ off,
                                                            const int* __restrict__ sorted, const float* __restrict__ wgt,
                                                            float* __restrict__ dx, int c, int plane) {
  const int cell = blockIdx.x * 256 + threadIdx.x, cc = blockIdx.y, bn = blockIdx.z;
  if (cell >= plane) return;
  const int E = 4 * plane;
  const int* o = off + (size_t)bn * (plane + 1);
  const int lo = o[cell], hi = o[cell + 1];
  const int* l = sorted + (size_t)bn * E;
  const float* wg = wgt + (size_t)bn * E;
  const float* g = dout + ((size_t)bn * c + cc) * plane;
  float v = 0.f;
  for (int j = lo; j < hi; ++j) {
    const int k = l[j];
    v += g[k >> 2] * wg[k];
  }
  dx[((size_t)bn * c + cc) * plane + cell] = v;
}

// ---- step 1 for DCNv2 (64 channels, 8 deformable groups, 3 x 3, stride / pad / dilation 1): the sampling rule of dcn_bwd.hip's b_samp
// (validity -1 < p < size, corner-wise zero padding).  Source = (tap, pixel), segment = (sample, group).
constexpr int D_DG = 8;
__global__ __launch_bounds__(256) void dcn_det_sample_kernel(const float* __restrict__ offset, int* __restrict__ dst, float* __restrict__ wgt,
                                                             int h, int w) {
  const int hw = h * w;
  const int p = blockIdx.x * 256 + threadIdx.x, tap = blockIdx.y, sg = blockIdx.z;      // sg = bn * 8 + g
  if (p >= hw) return;
  const int gy = p / w, gx = p - gy * w;
  const size_t oi = ((size_t)sg * 18 + 2 * tap) * hw + p;
  const float py = eavsr_sample_pos((float)(gy - 1 + tap / 3) + offset[oi], h);
  const float px = eavsr_sample_pos((float)(gx - 1 + tap % 3) + offset[oi + hw], w);
  const bool in = py > -1.f && px > -1.f && py < (float)h && px < (float)w;
  const float fy0 = floorf(py), fx0 = floorf(px);
  const float lh = py - fy0, lw = px - fx0, hh = 1.f - lh, hwt = 1.f - lw;
  const int hl = (int)fminf(fmaxf(fy0, -2.f), (float)h), wl = (int)fminf(fmaxf(fx0, -2.f), (float)w);
  const int hh_i = hl + 1, wh_i = wl + 1;
  const bool t_ok = hl >= 0, b_ok = hh_i <= h - 1, l_ok = wl >= 0, r_ok = wh_i <= w - 1;
  const size_t e = ((size_t)sg * 9 * hw + (size_t)tap * hw + p) * 4;
  dst[e + 0] = in && t_ok && l_ok ? hl * w + wl : -1;
  dst[e + 1] = in && t_ok && r_ok ? hl * w + wh_i : -1;
  dst[e + 2] = in && b_ok && l_ok ? hh_i * w + wl : -1;
  dst[e + 3] = in && b_ok && r_ok ? hh_i * w + wh_i : -1;
  wgt[e + 0] = hh * hwt;
  wgt[e + 1] = hh * lw;
  wgt[e + 2] = lh * hwt;
  wgt[e + 3] = lh * lw;
}

// ---- step 6 for DCNv2: dx[bn][g * 8 + c][cell] = sum over the cell's list, in key order, of (dcol * mask) * weight, with
// dcol = dcolumns[bn][(g * 8 + c) * 9 + tap][pixel] (the 576-row column gradient W^T . dY) and mask[bn][g * 9 + tap][pixel]
__global__ __launch_bounds__(256) void dcn_det_gather_kernel(const float* __restrict__ dcol, const float* __restrict__ mask,
                                                             const int* __restrict__ off, const int* __restrict__ sorted,
                                                             const float* __restrict__ wgt, float* __restrict__ dx, int hw) {
  const int cell = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, sg = blockIdx.z;
  if (cell >= hw) return;
  const int bn = sg / D_DG, g = sg - bn * D_DG;
  const int E = 36 * hw;
  const int* o = off + (size_t)sg * (hw + 1);
  const int lo = o[cell], hi = o[cell + 1];
  const int* l = sorted + (size_t)sg * E;
  const float* wg = wgt + (size_t)sg * E;
  const float* dc = dcol + ((size_t)bn * 576 + (size_t)(g * 8 + c) * 9) * hw;
  const float* m = mask + ((size_t)bn * 72 + (size_t)g * 9) * hw;
  float v = 0.f;
  for (int j = lo; j < hi; ++j) {
    const int k = l[j], src = k >> 2;      // src = tap * hw + pixel
    v += (dc[src] * m[src]) * wg[k];
  }
  dx[((size_t)bn * 64 + g * 8 + c) * hw + cell] = v;
}

// ---- resize_bilinear_ac backward as a gather
// the output indices o whose corner 0 or 1 (along one axis) can be input index i: an analytic window, filtered exactly by the caller
__device__ __forceinline__ void rs_window(int i, int nin, int nout, float r, int& lo, int& hi) {
  if (!(r > 0.f)) {      // nout == 1 or nin == 1: every output samples position 0
    lo = 0; hi = nout - 1;
    return;
  }
  lo = max(0, (int)floorf((float)(i - 1) / r) - 2);
  hi = i >= nin - 1 ? nout - 1 : min(nout - 1, (int)ceilf((float)(i + 1) / r) + 2);
}

__global__ __launch_bounds__(256) void resize_ac_bwd_det_kernel(const float* __restrict__ dout, float* __restrict__ din, int hin, int win,
                                                                int hout, int wout, float rh, float rw, float scale) {
  const int ix = blockIdx.x * 64 + threadIdx.x;
  const int iy = blockIdx.y * 4 + threadIdx.y;
  const int nc = blockIdx.z;
  if (ix >= win || iy >= hin) return;
  int ylo, yhi, xlo, xhi;
  rs_window(iy, hin, hout, rh, ylo, yhi);
  rs_window(ix, win, wout, rw, xlo, xhi);
  const float* g = dout + (size_t)nc * hout * wout;
  float v = 0.f;
  for (int oy = ylo; oy <= yhi; ++oy) {
    const float sy = rh * (float)oy;
    const int y0 = min((int)sy, hin - 1);
    const int y1 = y0 + (y0 < hin - 1 ? 1 : 0);
    if (y0 != iy && y1 != iy) continue;
    const float ly1 = sy - (float)y0, ly0 = 1.f - ly1;
    for (int ox = xlo; ox <= xhi; ++ox) {
      const float sx = rw * (float)ox;
      const int x0 = min((int)sx, win - 1);
      const int x1 = x0 + (x0 < win - 1 ? 1 : 0);
      if (x0 != ix && x1 != ix) continue;
      const float lx1 = sx - (float)x0, lx0 = 1.f - lx1;
      const float gv = g[(size_t)oy * wout + ox] * scale;
      // the atomic kernel's four terms, in its corner order
      if (y0 == iy && x0 == ix) v += gv * ly0 * lx0;
      if (y0 == iy && x1 == ix) v += gv * ly0 * lx1;
      if (y1 == iy && x0 == ix) v += gv * ly1 * lx0;
      if (y1 == iy && x1 == ix) v += gv * ly1 * lx1;
    }
  }
  din[(size_t)nc * hin * win + (size_t)iy * win + ix] = v;
}

// workspace words (4 bytes each) of one index: dst, wgt, list, sorted (E per segment), off (ncell + 1), cur (ncell)
int64_t index_words(int64_t segs, int64_t E, int64_t ncell) { return segs * (4 * E + 2 * ncell + 1); }

// steps 2-5 on a workspace whose dst / wgt step 1 has written
int build_index(int* dst, int* off, int* cur, int* list, int* sorted, int segs, int E, int ncell, hipStream_t st) {
  // (zeroed by a kernel: off and cur are adjacent, one launch; a kernel is captured into a graph like every other launch)
  const long words = (long)segs * (2 * ncell + 1);
  hipLaunchKernelGGL(ds_zero_kernel, dim3((unsigned)std::min<long>((words + 255) / 256, 4096)), dim3(256), 0, st, off, words);
  const dim3 grid(eavsr::cdiv(E, 256), segs);
  hipLaunchKernelGGL(ds_count_kernel, grid, dim3(256), 0, st, dst, off, E, ncell);
  hipLaunchKernelGGL(ds_scan_kernel, dim3(segs), dim3(1024), 0, st, off, ncell);
  hipLaunchKernelGGL(ds_fill_kernel, grid, dim3(256), 0, st, dst, off, cur, list, E, ncell);
  hipLaunchKernelGGL(ds_rank_kernel, grid, dim3(256), 0, st, dst, off, list, sorted, E, ncell);
  return eavsr::launch_status("det_index");
}

}  // namespace

extern "C" int64_t eavsr_flow_warp_bwd_dx_det_workspace_floats(int32_t n, int32_t h, int32_t w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return index_words(n, 4 * (int64_t)h * w, (int64_t)h * w);
}

extern "C" int eavsr_flow_warp_bwd_dx_det_f32(const float* flow, const float* flow2, const float* dout, float* dx, void* workspace,
                                              int32_t n, int32_t c, int32_t h, int32_t w, void* stream) {
  EAVSR_REQUIRE(flow && dout && dx && workspace, -1, "flow_warp_bwd_dx_det: NULL pointer");
  EAVSR_REQUIRE(n >= 0 && c >= 0 && h > 0 && w > 0 && n <= 65535 && c <= 65535 && 4L * h * w < (1L << 31), -1,
                "flow_warp_bwd_dx_det: bad dims");
  if (n == 0 || c == 0) return 0;
  hipStream_t st = eavsr::as_stream(stream);
  const int plane = h * w, E = 4 * plane;
  int* dst = static_cast<int*>(workspace);
  float* wgt = reinterpret_cast<float*>(dst + (size_t)n * E);
  int* list = reinterpret_cast<int*>(wgt + (size_t)n * E);
  int* sorted = list + (size_t)n * E;
  int* off = sorted + (size_t)n * E;
  int* cur = off + (size_t)n * (plane + 1);
  hipLaunchKernelGGL(fw_det_sample_kernel, dim3(eavsr::cdiv(plane, 256), n), dim3(256), 0, st, flow, flow2, dst, wgt, h, w);
  const int r = build_index(dst, off, cur, list, sorted, n, E, plane, st);
  if (r != 0) return r;
  hipLaunchKernelGGL(fw_det_gather_kernel, dim3(eavsr::cdiv(plane, 256), c, n), dim3(256), 0, st, dout, off, sorted, wgt, dx, c, plane);
  return eavsr::launch_status("flow_warp_bwd_dx_det");
}

extern "C" int64_t eavsr_dcnv2_col2im_dx_det_workspace_floats(int32_t n, int32_t h, int32_t w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return index_words((int64_t)n * D_DG, 36 * (int64_t)h * w, (int64_t)h * w);
}

extern "C" int eavsr_dcnv2_col2im_dx_det_f32(const float* offset, const float* mask, const float* dcolumns, float* dx, void* workspace,
                                             int32_t n, int32_t c, int32_t h, int32_t w, int32_t deform_groups, void* stream) {
  EAVSR_REQUIRE(offset && mask && dcolumns && dx && workspace, -1, "dcnv2_col2im_dx_det: NULL pointer");
  EAVSR_REQUIRE(c == 64 && deform_groups == D_DG, -2, "dcnv2_col2im_dx_det: 64 channels in 8 deformable groups (got %d, %d groups)", c,
                deform_groups);
  EAVSR_REQUIRE(n >= 0 && h > 0 && w > 0 && (long)n * D_DG <= 65535 && 36L * h * w < (1L << 31), -1, "dcnv2_col2im_dx_det: bad dims");
  if (n == 0) return 0;
  hipStream_t st = eavsr::as_stream(stream);
  const int hw = h * w, E = 36 * hw, segs = n * D_DG;
  int* dst = static_cast<int*>(workspace);
  float* wgt = reinterpret_cast<float*>(dst + (size_t)segs * E);
  int* list = reinterpret_cast<int*>(wgt + (size_t)segs * E);
  int* sorted = list + (size_t)segs * E;
  int* off = sorted + (size_t)segs * E;
  int* cur = off + (size_t)segs * (hw + 1);
  hipLaunchKernelGGL(dcn_det_sample_kernel, dim3(eavsr::cdiv(hw, 256), 9, segs), dim3(256), 0, st, offset, dst, wgt, h, w);
  const int r = build_index(dst, off, cur, list, sorted, segs, E, hw, st);
  if (r != 0) return r;
  hipLaunchKernelGGL(dcn_det_gather_kernel, dim3(eavsr::cdiv(hw, 256), 8, segs), dim3(256), 0, st, dcolumns, mask, off, sorted, wgt, dx, hw);
  return eavsr::launch_status("dcnv2_col2im_dx_det");
}

extern "C" int eavsr_resize_bilinear_ac_bwd_det_f32(const float* dout, float* din, int32_t n, int32_t c, int32_t hin, int32_t win,
                                                    int32_t hout, int32_t wout, float scale, void* stream) {
  EAVSR_REQUIRE(dout && din, -1, "resize_bilinear_ac_bwd_det: NULL pointer");
  EAVSR_REQUIRE(n >= 0 && c >= 0 && hin > 0 && win > 0 && hout > 0 && wout > 0 && (long)n * c <= 65535, -1,
                "resize_bilinear_ac_bwd_det: bad dims");
  if (n * c == 0) return 0;
  const float rh = hout > 1 ? (float)(hin - 1) / (float)(hout - 1) : 0.f;
  const float rw = wout > 1 ? (float)(win - 1) / (float)(wout - 1) : 0.f;
  dim3 grid(eavsr::cdiv(win, 64), eavsr::cdiv(hin, 4), n * c), block(64, 4, 1);
  hipLaunchKernelGGL(resize_ac_bwd_det_kernel, grid, block, 0, eavsr::as_stream(stream), dout, din, hin, win, hout, wout, rh, rw, scale);
  return eavsr::launch_status("resize_bilinear_ac_bwd_det");
}
