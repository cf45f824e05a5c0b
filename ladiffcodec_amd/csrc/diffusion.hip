// diffusion.hip -- layout changes at the ABI boundary, max-abs scaling, the fused p_sample update,
// the device-resident step counter, Philox noise and the output normalisation.
//
//   p_sample arithmetic  : reference srcs/losses/ddpm_loss.py:175-179 (x0 from eps), :237-238 (clamp),
//                          :199-206 (posterior mean), :249-250 (noise unless t == 0)
//   ddim_update          : ddpm_loss.py:268-303 (ddim_sample, clip_denoised); coefficients per iteration from the host
//   max-abs scaling      : unet.py:401-403 (per item, +1e-20) and sample.py:129 (whole tensor, +1e-8)
//   output normalisation : sample.py:133-134
// All kernels here are HBM-bound: p_sample_update moves 4 fp32 reads/writes + 2 dtype accesses per
// element of [B,128,L].
#include <algorithm>

#include "ldc_kernels.h"
#include "ldc_math.h"

namespace ldc {

__device__ __forceinline__ float dbf2f(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }
__device__ __forceinline__ unsigned short df2bf(float f) { return hw_bf16(f); }
template <typename T>
__device__ __forceinline__ float dld(const void* p, size_t i);
template <>
__device__ __forceinline__ float dld<float>(const void* p, size_t i) { return reinterpret_cast<const float*>(p)[i]; }
template <>
__device__ __forceinline__ float dld<__bf16>(const void* p, size_t i) {
  return dbf2f(reinterpret_cast<const unsigned short*>(p)[i]);
}
template <typename T>
__device__ __forceinline__ void dst(void* p, size_t i, float v);
template <>
__device__ __forceinline__ void dst<float>(void* p, size_t i, float v) { reinterpret_cast<float*>(p)[i] = v; }
template <>
__device__ __forceinline__ void dst<__bf16>(void* p, size_t i, float v) {
  reinterpret_cast<unsigned short*>(p)[i] = df2bf(v);
}

// ---------------------------------------------------------------------------------------------
// [B][C][L] f32  <->  [B][L][C] dt through a 32x32 LDS tile (both sides coalesced)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void to_cl_kernel(const float* x, void* y, int C, int L, const float* maxabs,
                                                    int per_item, float eps) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, l0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float den = 1.0f;
  if (maxabs) den = maxabs[per_item ? b : 0] + eps;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, l = l0 + tx;
    tile[i][tx] = (c < C && l < L) ? x[((size_t)b * C + c) * L + l] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int l = l0 + i, c = c0 + tx;
    if (l < L && c < C) {
      float v = tile[tx][i];
      if (maxabs) v = v / den;
      dst<T>(y, ((size_t)b * L + l) * C + c, v);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void from_cl_kernel(const void* x, float* y, int C, int L, const float* maxabs,
                                                      int per_item, float eps) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, l0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float den = 1.0f;
  if (maxabs) den = maxabs[per_item ? b : 0] + eps;
  for (int i = ty; i < 32; i += 8) {
    const int l = l0 + i, c = c0 + tx;
    tile[i][tx] = (c < C && l < L) ? dld<T>(x, ((size_t)b * L + l) * C + c) : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, l = l0 + tx;
    if (l < L && c < C) {
      float v = tile[tx][i];
      if (maxabs) v = v / den;
      y[((size_t)b * C + c) * L + l] = v;
    }
  }
}

hipError_t launch_to_cl(int dt, const float* x, void* y, int B, int C, int L, const float* maxabs, int per_item,
                        float eps, hipStream_t s) {
  dim3 grid((L + 31) / 32, (C + 31) / 32, B);
  if (dt == DT_F32)
    hipLaunchKernelGGL(to_cl_kernel<float>, grid, dim3(256), 0, s, x, y, C, L, maxabs, per_item, eps);
  else
    hipLaunchKernelGGL(to_cl_kernel<__bf16>, grid, dim3(256), 0, s, x, y, C, L, maxabs, per_item, eps);
  return hipGetLastError();
}

hipError_t launch_from_cl(int dt, const void* x, float* y, int B, int C, int L, const float* maxabs, int per_item,
                          float eps, hipStream_t s) {
  dim3 grid((L + 31) / 32, (C + 31) / 32, B);
  if (dt == DT_F32)
    hipLaunchKernelGGL(from_cl_kernel<float>, grid, dim3(256), 0, s, x, y, C, L, maxabs, per_item, eps);
  else
    hipLaunchKernelGGL(from_cl_kernel<__bf16>, grid, dim3(256), 0, s, x, y, C, L, maxabs, per_item, eps);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// max |x| per item (or global).  |x| >= 0, so the raw float bits order like unsigned ints.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxabs_kernel(const void* x, int64_t n_per_item, int per_item, float* maxabs) {
  const int b = blockIdx.y;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_per_item; i += (int64_t)gridDim.x * 256)
    m = fmaxf(m, fabsf(dld<T>(x, (size_t)b * n_per_item + i)));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(reinterpret_cast<unsigned*>(maxabs) + (per_item ? b : 0), __float_as_uint(m));
  }
}

hipError_t launch_maxabs(int dt, const void* x, int B, int64_t n_per_item, int per_item, float* maxabs, hipStream_t s) {
  int bx = (int)std::min<int64_t>((n_per_item + 255) / 256, 64);
  if (bx < 1) bx = 1;
  if (dt == DT_F32)
    hipLaunchKernelGGL(maxabs_kernel<float>, dim3(bx, B), dim3(256), 0, s, x, n_per_item, per_item, maxabs);
  else
    hipLaunchKernelGGL(maxabs_kernel<__bf16>, dim3(bx, B), dim3(256), 0, s, x, n_per_item, per_item, maxabs);
  return hipGetLastError();
}

template <typename T>
__global__ __launch_bounds__(256) void scale_by_maxabs_kernel(void* x, int64_t n_per_item, const float* maxabs,
                                                              int per_item, float eps) {
  const int b = blockIdx.y;
  const float den = maxabs[per_item ? b : 0] + eps;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_per_item; i += (int64_t)gridDim.x * 256) {
    const size_t idx = (size_t)b * n_per_item + i;
    dst<T>(x, idx, dld<T>(x, idx) / den);
  }
}

hipError_t launch_scale_by_maxabs(int dt, void* x, int B, int64_t n_per_item, const float* maxabs, int per_item,
                                  float eps, hipStream_t s) {
  int bx = (int)std::min<int64_t>((n_per_item + 255) / 256, 256);
  if (bx < 1) bx = 1;
  if (dt == DT_F32)
    hipLaunchKernelGGL(scale_by_maxabs_kernel<float>, dim3(bx, B), dim3(256), 0, s, x, n_per_item, maxabs, per_item, eps);
  else
    hipLaunchKernelGGL(scale_by_maxabs_kernel<__bf16>, dim3(bx, B), dim3(256), 0, s, x, n_per_item, maxabs, per_item, eps);
  return hipGetLastError();
}

// y = x / (maxabs[b] + eps), out of place (--unet_scale_x: the UNet input scaled per item, unet.py:432-433)
template <typename T>
__global__ __launch_bounds__(256) void scale_copy_kernel(const void* x, void* y, int64_t n_per_item, const float* maxabs, float eps) {
  const int b = blockIdx.y;
  const float den = maxabs[b] + eps;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_per_item; i += (int64_t)gridDim.x * 256) {
    const size_t idx = (size_t)b * n_per_item + i;
    dst<T>(y, idx, dld<T>(x, idx) / den);
  }
}
hipError_t launch_scale_copy(int dt, const void* x, void* y, int B, int64_t n_per_item, const float* maxabs, float eps, hipStream_t s) {
  int bx = (int)std::min<int64_t>((n_per_item + 255) / 256, 256);
  if (bx < 1) bx = 1;
  if (dt == DT_F32) hipLaunchKernelGGL(scale_copy_kernel<float>, dim3(bx, B), dim3(256), 0, s, x, y, n_per_item, maxabs, eps);
  else hipLaunchKernelGGL(scale_copy_kernel<__bf16>, dim3(bx, B), dim3(256), 0, s, x, y, n_per_item, maxabs, eps);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 + Box-Muller: one normal per (seed, step, element)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned (&k)[2]) {
  const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
  const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
  const unsigned c0 = (unsigned)(p1 >> 32) ^ c[1] ^ k[0];
  const unsigned c2 = (unsigned)(p0 >> 32) ^ c[3] ^ k[1];
  c[1] = (unsigned)p1; c[3] = (unsigned)p0; c[0] = c0; c[2] = c2;
  k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
}
__device__ __forceinline__ float philox_normal(uint64_t seed, unsigned step, uint64_t elem) {
  unsigned c[4] = {(unsigned)elem, (unsigned)(elem >> 32), step, 0x4c444321u};
  unsigned k[2] = {(unsigned)seed, (unsigned)(seed >> 32)};
#pragma unroll
  for (int i = 0; i < 10; ++i) philox_round(c, k);
  const float u1 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);   // (0,1]
  const float u2 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);            // [0,1)
  return sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530717958647692f * u2);
}

// four normals from one Philox block: both Box-Muller branches of two (u1, u2) pairs
__device__ __forceinline__ void philox_normal4(uint64_t seed, unsigned step, uint64_t group, float (&z)[4]) {
  unsigned c[4] = {(unsigned)group, (unsigned)(group >> 32), step, 0x4c444323u};
  unsigned k[2] = {(unsigned)seed, (unsigned)(seed >> 32)};
#pragma unroll
  for (int i = 0; i < 10; ++i) philox_round(c, k);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(c[2 * h] >> 8) + 1.0f) * (1.0f / 16777216.0f);   // (0,1]
    const float u2 = (float)(c[2 * h + 1] >> 8) * (1.0f / 16777216.0f);        // [0,1)
    const float r = sqrtf(-2.0f * __logf(u1));
    float sn, cs;
    __sincosf(6.28318530717958647692f * u2, &sn, &cs);
    z[2 * h] = r * cs;
    z[2 * h + 1] = r * sn;
  }
}

// ---------------------------------------------------------------------------------------------
// The samplers' arithmetic on one element, shared by every update kernel that applies it (whole batches, windows):
//   x0 = clamp(sqrt_recip_ac[t] x - sqrt_recipm1_ac[t] eps, -1, 1)                (ddpm_loss.py:175-179, :237-238)
//   p_sample : c1 x0 + c2 x  (the posterior mean, :199-206; the caller adds sigma z unless t == 0)
//   DDIM     : last ? x0 : x0 sqrt_an + c eps  (:268-303; the caller adds sigma z where the entry draws)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float clipped_x0(float recip, float recipm1, float xv, float e) {
  const float x0 = recip * xv - recipm1 * e;
  return fminf(fmaxf(x0, -1.0f), 1.0f);
}
__device__ __forceinline__ float p_sample_mean(float recip, float recipm1, float c1, float c2, float xv, float e) {
  const float x0 = clipped_x0(recip, recipm1, xv, e);
  return c1 * x0 + c2 * xv;
}
__device__ __forceinline__ float ddim_mean(const DdimStep& sp, float recip, float recipm1, float xv, float e) {
  const float x0 = clipped_x0(recip, recipm1, xv, e);
  float v = x0;
  if (!sp.last) v = x0 * sp.sqrt_an + sp.c * e;
  return v;
}

// ---------------------------------------------------------------------------------------------
// p_sample update on [B][C][L] fp32 state, eps arriving channels-last; also emits the channels-last
// copy of the new state for the next UNet call.  Tile: 32 positions x 32 channels.
// ---------------------------------------------------------------------------------------------
// ITEM (the item-seeded form, DESIGN.md section 5e "Item seeds"): the Philox key of item blockIdx.z is item_keys[blockIdx.z] (the part's
// key table, launch_item_keys_write) instead of the step state's, and the block index is the one of the item ALONE on its own length,
// (c0 + ty) * Lv + l -- what p_sample_update_items_kernel draws -- so neither elem_base, the item's position nor the padded length enter.
template <typename T, bool ITEM>
__device__ __forceinline__ void p_sample_update_body(float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride, void* x_cl,
                                                     int C, int L, const StepTables& tb, const int* st, uint64_t elem_base, const int* lens,
                                                     const uint64_t* item_keys) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, l0 = blockIdx.x * 32;
  const int Lv = valid_rows(lens, 0, b, L);   // ragged batch: positions [Lv, L) are padding -- x stays zero there, their noise is not read
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  // the tensor loads do not depend on the step: issue them before the (dependent) step-counter -> schedule-table chain
  // eps tile: read channels-last (coalesced over c), hand over transposed
  float ev[4], xin[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int l = l0 + i, c = c0 + tx;
    ev[ii] = (l < L && c < C) ? dld<T>(eps_cl, ((size_t)b * L + l) * C + c) : 0.f;
    const int cc = c0 + i, ll = l0 + tx;
    xin[ii] = (cc < C && ll < L) ? x[((size_t)b * C + cc) * L + ll] : 0.f;
  }
  const int t = st[0], j = st[1];
  const uint64_t seed = ITEM ? item_keys[b] : ((uint64_t)(unsigned)st[3] << 32) | (uint64_t)(unsigned)st[2];   // (the key rides with the step words, in front of the table chain)
  const float recip = tb.sqrt_recip_alphas_cumprod[t], recipm1 = tb.sqrt_recipm1_alphas_cumprod[t];
  const float c1 = tb.posterior_mean_coef1[t], c2 = tb.posterior_mean_coef2[t];
  const float sigma = expf(0.5f * tb.posterior_log_variance_clipped[t]);
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = ev[ii];
  __syncthreads();
  float newv[4];
  // the thread's four elements (channels c0+ty+{0,8,16,24}, one position) share one Philox block; the block index is
  // the global index of the first of them, so the draws do not depend on how the batch is split
  float zz[4] = {0.f, 0.f, 0.f, 0.f};
  if (t > 0 && !noise)
    philox_normal4(seed, (unsigned)j, ITEM ? (uint64_t)(c0 + ty) * Lv + l0 + tx : elem_base + ((size_t)b * C + c0 + ty) * L + l0 + tx, zz);
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int c = c0 + i, l = l0 + tx;
    newv[ii] = 0.f;
    if (c < C && l < L) {
      const size_t idx = ((size_t)b * C + c) * L + l;
      const float xv = xin[ii];
      const float e = tile[tx][i];
      float v = p_sample_mean(recip, recipm1, c1, c2, xv, e);
      if (t > 0 && l < Lv) {
        const float z = noise ? noise[(size_t)j * noise_step_stride + idx] : zz[ii];
        v += sigma * z;
      }
      v = l < Lv ? v : 0.f;
      x[idx] = v;
      newv[ii] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = newv[ii];   // tile[c][l]
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int l = l0 + i, c = c0 + tx;
    if (l < L && c < C) dst<T>(x_cl, ((size_t)b * L + l) * C + c, tile[tx][i]);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void p_sample_update_kernel(float* x, const void* eps_cl, const float* noise,
                                                              int64_t noise_step_stride, void* x_cl, int C, int L,
                                                              StepTables tb, const int* st, uint64_t elem_base, const int* lens) {
  p_sample_update_body<T, false>(x, eps_cl, noise, noise_step_stride, x_cl, C, L, tb, st, elem_base, lens, nullptr);
}
template <typename T>
__global__ __launch_bounds__(256) void p_sample_update_seeded_kernel(float* x, const void* eps_cl, const float* noise,
                                                                     int64_t noise_step_stride, void* x_cl, int C, int L, StepTables tb,
                                                                     const int* st, const int* lens, const uint64_t* item_keys) {
  p_sample_update_body<T, true>(x, eps_cl, noise, noise_step_stride, x_cl, C, L, tb, st, 0, lens, item_keys);
}

// start images of the alternative samplers: standard normal (p_sample_loop, ddpm_loss.py:257) or uniform [0,1)
// (infilling, ddpm_loss.py:336) from the same counter-based generator; stream `step` keeps them apart from the
// per-step noise draws
__global__ __launch_bounds__(256) void random_fill_kernel(float* x, int64_t n, int uniform, uint64_t seed, unsigned step) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (uniform) {
      unsigned c[4] = {(unsigned)i, (unsigned)((uint64_t)i >> 32), step, 0x4c444322u};
      unsigned k[2] = {(unsigned)seed, (unsigned)(seed >> 32)};
#pragma unroll
      for (int r = 0; r < 10; ++r) philox_round(c, k);
      x[i] = (float)(c[0] >> 8) * (1.0f / 16777216.0f);
    } else {
      x[i] = philox_normal(seed, step, (uint64_t)i);
    }
  }
}
hipError_t launch_random_fill(float* x, int64_t n, int uniform, uint64_t seed, unsigned step, hipStream_t s) {
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(random_fill_kernel, dim3(std::max(1, blocks)), dim3(256), 0, s, x, n, uniform, seed, step);
  return hipGetLastError();
}

// x = a*x + b*y (the blends of infilling, ddpm_loss.py:357,361)
__global__ __launch_bounds__(256) void axpby_kernel(float* x, const float* y, float a, float b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = a * x[i] + b * y[i];
}
hipError_t launch_axpby(float* x, const float* y, float a, float b, int64_t n, hipStream_t s) {
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(axpby_kernel, dim3(std::max(1, blocks)), dim3(256), 0, s, x, y, a, b, n);
  return hipGetLastError();
}

hipError_t launch_p_sample_update(int dt, float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride,
                                  void* x_cl, int B, int C, int L, StepTables tb, const int* st,
                                  uint64_t elem_base, hipStream_t s, const int* lens, const uint64_t* item_keys) {
  dim3 grid((L + 31) / 32, (C + 31) / 32, B);
  if (item_keys) {   // the item-seeded form: keys from the part's table, block indices of the item alone (elem_base does not enter)
    if (dt == DT_F32)
      hipLaunchKernelGGL(p_sample_update_seeded_kernel<float>, grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, C, L, tb, st,
                         lens, item_keys);
    else
      hipLaunchKernelGGL(p_sample_update_seeded_kernel<__bf16>, grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, C, L, tb, st,
                         lens, item_keys);
    return hipGetLastError();
  }
  if (dt == DT_F32)
    hipLaunchKernelGGL(p_sample_update_kernel<float>, grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, C, L,
                       tb, st, elem_base, lens);
  else
    hipLaunchKernelGGL(p_sample_update_kernel<__bf16>, grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, C,
                       L, tb, st, elem_base, lens);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// DDIM update (ddpm_loss.py ddim_sample with clip_denoised): the p_sample_update tiling, coefficients of iteration
// j = st[1] from the host-written schedule table.  x0 uses eps as the UNet returned it (the reference does not
// re-derive pred_noise from the clipped x0).
// ---------------------------------------------------------------------------------------------
// ITEM: the item-seeded form, as p_sample_update_body's
template <typename T, bool ITEM>
__device__ __forceinline__ void ddim_update_body(float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride, void* x_cl, int C,
                                                 int L, const StepTables& tb, const DdimStep* sched, const int* st, uint64_t elem_base,
                                                 const int* lens, const uint64_t* item_keys) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, l0 = blockIdx.x * 32;
  const int Lv = valid_rows(lens, 0, b, L);   // as p_sample_update_kernel
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float ev[4], xin[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int l = l0 + i, c = c0 + tx;
    ev[ii] = (l < L && c < C) ? dld<T>(eps_cl, ((size_t)b * L + l) * C + c) : 0.f;
    const int cc = c0 + i, ll = l0 + tx;
    xin[ii] = (cc < C && ll < L) ? x[((size_t)b * C + cc) * L + ll] : 0.f;
  }
  const int j = st[1];
  const uint64_t seed = ITEM ? item_keys[b] : ((uint64_t)(unsigned)st[3] << 32) | (uint64_t)(unsigned)st[2];
  const DdimStep sp = sched[j];
  const float recip = tb.sqrt_recip_alphas_cumprod[sp.t], recipm1 = tb.sqrt_recipm1_alphas_cumprod[sp.t];
  const bool draw = !sp.last && sp.sigma > 0.f;
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = ev[ii];
  __syncthreads();
  float newv[4];
  // one Philox block per thread at the global index of its first element, as in p_sample_update_kernel
  float zz[4] = {0.f, 0.f, 0.f, 0.f};
  if (draw && !noise)
    philox_normal4(seed, (unsigned)j, ITEM ? (uint64_t)(c0 + ty) * Lv + l0 + tx : elem_base + ((size_t)b * C + c0 + ty) * L + l0 + tx, zz);
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int c = c0 + i, l = l0 + tx;
    newv[ii] = 0.f;
    if (c < C && l < L) {
      const size_t idx = ((size_t)b * C + c) * L + l;
      const float e = tile[tx][i];
      float v = ddim_mean(sp, recip, recipm1, xin[ii], e);
      if (draw && l < Lv) v += sp.sigma * (noise ? noise[(size_t)j * noise_step_stride + idx] : zz[ii]);   // (draw: not the last iteration)
      v = l < Lv ? v : 0.f;
      x[idx] = v;
      newv[ii] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = newv[ii];   // tile[c][l]
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int l = l0 + i, c = c0 + tx;
    if (l < L && c < C) dst<T>(x_cl, ((size_t)b * L + l) * C + c, tile[tx][i]);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void ddim_update_kernel(float* x, const void* eps_cl, const float* noise,
                                                          int64_t noise_step_stride, void* x_cl, int C, int L,
                                                          StepTables tb, const DdimStep* sched, const int* st,
                                                          uint64_t elem_base, const int* lens) {
  ddim_update_body<T, false>(x, eps_cl, noise, noise_step_stride, x_cl, C, L, tb, sched, st, elem_base, lens, nullptr);
}
template <typename T>
__global__ __launch_bounds__(256) void ddim_update_seeded_kernel(float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride,
                                                                 void* x_cl, int C, int L, StepTables tb, const DdimStep* sched, const int* st,
                                                                 const int* lens, const uint64_t* item_keys) {
  ddim_update_body<T, true>(x, eps_cl, noise, noise_step_stride, x_cl, C, L, tb, sched, st, 0, lens, item_keys);
}

hipError_t launch_ddim_update(int dt, float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride,
                              void* x_cl, int B, int C, int L, StepTables tb, const DdimStep* sched, const int* st,
                              uint64_t elem_base, hipStream_t s, const int* lens, const uint64_t* item_keys) {
  dim3 grid((L + 31) / 32, (C + 31) / 32, B);
  if (item_keys) {   // the item-seeded form, as launch_p_sample_update's
    if (dt == DT_F32)
      hipLaunchKernelGGL(ddim_update_seeded_kernel<float>, grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, C, L, tb, sched, st,
                         lens, item_keys);
    else
      hipLaunchKernelGGL(ddim_update_seeded_kernel<__bf16>, grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, C, L, tb, sched,
                         st, lens, item_keys);
    return hipGetLastError();
  }
  if (dt == DT_F32)
    hipLaunchKernelGGL(ddim_update_kernel<float>, grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, C, L,
                       tb, sched, st, elem_base, lens);
  else
    hipLaunchKernelGGL(ddim_update_kernel<__bf16>, grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, C,
                       L, tb, sched, st, elem_base, lens);
  return hipGetLastError();
}

// the DDIM schedule table written on the stream (kernel arguments carry the entries: no host buffer outlives the call)
constexpr int kDdimChunk = 64;
struct DdimChunk { DdimStep e[kDdimChunk]; };
__global__ void ddim_table_write_kernel(DdimStep* dst, DdimChunk src, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = src.e[threadIdx.x];
}
hipError_t launch_ddim_table_write(DdimStep* dst, const DdimStep* src, int n, hipStream_t s) {
  for (int i0 = 0; i0 < n; i0 += kDdimChunk) {
    DdimChunk ch{};
    const int m = std::min(kDdimChunk, n - i0);
    for (int i = 0; i < m; ++i) ch.e[i] = src[i0 + i];
    hipLaunchKernelGGL(ddim_table_write_kernel, dim3(1), dim3(kDdimChunk), 0, s, dst + i0, ch, m);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// DPM-Solver++(2M) update, data-prediction form: the ddim_update tiling; coefficients of iteration
// j = st[1] from the host-written table.  x0_prev (the layout of x) is loaded only where the entry says has_prev and written
// on every iteration but the last; nothing is drawn.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dpm_update_kernel(float* x, const void* eps_cl, float* x0_prev, void* x_cl, int C, int L,
                                                         StepTables tb, const DpmStep* sched, const int* st, const int* lens) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, l0 = blockIdx.x * 32;
  const int Lv = valid_rows(lens, 0, b, L);   // as p_sample_update_kernel
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float ev[4], xin[4], pv[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int l = l0 + i, c = c0 + tx;
    ev[ii] = (l < L && c < C) ? dld<T>(eps_cl, ((size_t)b * L + l) * C + c) : 0.f;
    const int cc = c0 + i, ll = l0 + tx;
    xin[ii] = (cc < C && ll < L) ? x[((size_t)b * C + cc) * L + ll] : 0.f;
  }
  const DpmStep sp = sched[st[1]];
  const float recip = tb.sqrt_recip_alphas_cumprod[sp.t], recipm1 = tb.sqrt_recipm1_alphas_cumprod[sp.t];
  const bool hist = !sp.last && sp.has_prev;   // (uniform over the grid) the only case in which the history is read
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int cc = c0 + ty + ii * 8, ll = l0 + tx;
    pv[ii] = (hist && cc < C && ll < Lv) ? x0_prev[((size_t)b * C + cc) * L + ll] : 0.f;
  }
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = ev[ii];
  __syncthreads();
  float newv[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int c = c0 + i, l = l0 + tx;
    newv[ii] = 0.f;
    if (c < C && l < L) {
      const size_t idx = ((size_t)b * C + c) * L + l;
      const float e = tile[tx][i];
      float x0 = recip * xin[ii] - recipm1 * e;
      x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
      float v = x0;
      if (!sp.last) {
        v = sp.a * xin[ii] + sp.b0 * x0;
        if (hist) v += sp.b1 * pv[ii];
        x0_prev[idx] = l < Lv ? x0 : 0.f;
      }
      v = l < Lv ? v : 0.f;
      x[idx] = v;
      newv[ii] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = newv[ii];   // tile[c][l]
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int l = l0 + i, c = c0 + tx;
    if (l < L && c < C) dst<T>(x_cl, ((size_t)b * L + l) * C + c, tile[tx][i]);
  }
}

hipError_t launch_dpm_update(int dt, float* x, const void* eps_cl, float* x0_prev, void* x_cl, int B, int C, int L, StepTables tb,
                             const DpmStep* sched, const int* st, hipStream_t s, const int* lens) {
  dim3 grid((L + 31) / 32, (C + 31) / 32, B);
  if (dt == DT_F32)
    hipLaunchKernelGGL(dpm_update_kernel<float>, grid, dim3(256), 0, s, x, eps_cl, x0_prev, x_cl, C, L, tb, sched, st, lens);
  else
    hipLaunchKernelGGL(dpm_update_kernel<__bf16>, grid, dim3(256), 0, s, x, eps_cl, x0_prev, x_cl, C, L, tb, sched, st, lens);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Coupled windows: the overlapping windows of R recordings (a single-recording call is R = 1) are the items of
// ONE batch of the UNet; every recording keeps ONE fp32 state block that all its windows read, its own cover rows, noise and Philox
// key.  This kernel takes the place of the update launch of a step: the 32 x 32 tiling of p_sample_update_kernel over a recording's
// GLOBAL frames, walked over a host-built TILE TABLE -- blockIdx.x -> {recording, l0}, a recording owns ceil(Ltot_r / 32) tiles, so the
// recording of a tile is uniform over the workgroup and its table entry arrives through scalar loads.  A tile reads the cover entry
// (first window WITHIN the recording | count << 8, count <= 3, consecutive windows; the kernel adds w0_r) of each of its 32 frames,
// blends the covering windows' eps rows (channels-last, coalesced over c) with the host-built weights in fp32 and in window order -- a
// singly covered frame is 1.0f * eps --, applies the sampler's arithmetic to x as the B = 1, L = Ltot_r kernels above do, and stores
// the new state channels-last into the row of EVERY covering window of the UNet's input buffer.  x, the eps output, the history and
// the tape are packed, recording r's [C][Ltot_r] block at C * off_r floats, so the tape index and the Philox block of an element are
// those of the B = 1, L = Ltot_r call; the Philox key is the recording table's (launch_windows_group_keys), never the step state's.
// Frames of a recording's last tile at or behind Ltot_r have count 0: they blend nothing and are stored nowhere.  One writer per
// element of every window row (the tile that owns its global frame), no atomics.
// KIND WIN_BLEND stores the blended eps as packed [C][Ltot_r] fp32 and nothing else (ldc_unet_forward_windows / _windows_group).
// Load order: tile entry -> recording entry -> cover -> (start, weight, eps) and x do not depend on the step and are issued before the
// step state -> coefficient-table chain.  LDS: tile[32][33] fp32 -- rows written by 32 consecutive lanes, read transposed at stride
// 33 dwords: conflict-free.  All offsets size_t.
// ---------------------------------------------------------------------------------------------
template <typename T, int KIND>
__global__ __launch_bounds__(256) void windows_group_update_kernel(float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride,
                                                                   void* x_cl, float* ebar, int C, WinGroupTables gt, StepTables tb,
                                                                   const DdimStep* sched, const int* st) {
  __shared__ float tile[32][33];
  const WinGroupTile te = gt.tile[blockIdx.x];
  const WinGroupRec rc = gt.rec[te.rec];
  const int c0 = blockIdx.y * 32, l0 = te.l0;
  const int Ltot = rc.Ltot, Lw = gt.Lw, w0 = rc.w0;
  const size_t xo = (size_t)C * rc.off;   // the recording's block of x / ebar / the tape
  const int* cover = gt.cover + rc.cover_off;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  int cov[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int g = l0 + ty + ii * 8;
    cov[ii] = g < Ltot ? cover[g] : 0;   // (count 0: a frame behind the recording's end blends nothing and is stored nowhere)
  }
  float ev[4], xin[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int g = l0 + i, c = c0 + tx;
    const int first = w0 + (cov[ii] & 255), n = cov[ii] >> 8;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < n && c < C) {
        const int k = first + j, l = g - gt.start[k];
        const float we = gt.weight[(size_t)k * Lw + l] * dld<T>(eps_cl, ((size_t)k * Lw + l) * C + c);
        acc = j == 0 ? we : acc + we;
      }
    ev[ii] = acc;
    const int cc = c0 + i, ll = l0 + tx;
    xin[ii] = (KIND != WIN_BLEND && cc < C && ll < Ltot) ? x[xo + (size_t)cc * Ltot + ll] : 0.f;
  }
  int t = 0, j = 0;
  float recip = 0.f, recipm1 = 0.f, c1 = 0.f, c2 = 0.f, sigma = 0.f;
  DdimStep sp{};
  bool draw = false;
  if (KIND != WIN_BLEND) {
    t = st[0]; j = st[1];
    if (KIND == WIN_DDIM) { sp = sched[j]; t = sp.t; }
    recip = tb.sqrt_recip_alphas_cumprod[t]; recipm1 = tb.sqrt_recipm1_alphas_cumprod[t];
    if (KIND == WIN_DDPM) {
      c1 = tb.posterior_mean_coef1[t]; c2 = tb.posterior_mean_coef2[t];
      sigma = expf(0.5f * tb.posterior_log_variance_clipped[t]);
      draw = t > 0;
    } else {
      sigma = sp.sigma;
      draw = !sp.last && sp.sigma > 0.f;
    }
  }
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = ev[ii];
  __syncthreads();
  if (KIND == WIN_BLEND) {
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const int i = ty + ii * 8;
      const int c = c0 + i, g = l0 + tx;
      if (c < C && g < Ltot) ebar[xo + (size_t)c * Ltot + g] = tile[tx][i];
    }
    return;
  }
  float newv[4];
  // one Philox block per thread under the RECORDING's key at the index of its first element in the B = 1, L = Ltot_r layout
  float zz[4] = {0.f, 0.f, 0.f, 0.f};
  if (draw && !noise) philox_normal4(((uint64_t)rc.key_hi << 32) | (uint64_t)rc.key_lo, (unsigned)j, (uint64_t)(c0 + ty) * Ltot + l0 + tx, zz);
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int c = c0 + i, g = l0 + tx;
    newv[ii] = 0.f;
    if (c < C && g < Ltot) {
      const size_t idx = xo + (size_t)c * Ltot + g;
      const float e = tile[tx][i];
      float v = KIND == WIN_DDPM ? p_sample_mean(recip, recipm1, c1, c2, xin[ii], e) : ddim_mean(sp, recip, recipm1, xin[ii], e);
      if (draw) v += sigma * (noise ? noise[(size_t)j * noise_step_stride + idx] : zz[ii]);
      x[idx] = v;
      newv[ii] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = newv[ii];   // tile[c][g]
  __syncthreads();
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int g = l0 + i, c = c0 + tx;
    const int first = w0 + (cov[ii] & 255), n = cov[ii] >> 8;
    const float v = tile[tx][i];
#pragma unroll
    for (int jj = 0; jj < 3; ++jj)
      if (jj < n && c < C) {
        const int k = first + jj, l = g - gt.start[k];
        dst<T>(x_cl, ((size_t)k * Lw + l) * C + c, v);
      }
  }
}

static bool win_group_tables_ok(const WinGroupTables& gt) {
  return gt.n_tiles > 0 && gt.R > 0 && gt.Lw > 0 && gt.tile && gt.rec && gt.cover && gt.weight && gt.start && gt.wrec;
}

template <typename T>
static hipError_t launch_windows_group_update_t(int kind, float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride, void* x_cl,
                                                float* ebar, int C, WinGroupTables gt, StepTables tb, const DdimStep* sched, const int* st,
                                                hipStream_t s) {
  dim3 grid(gt.n_tiles, (C + 31) / 32, 1);
  if (kind == WIN_BLEND)
    hipLaunchKernelGGL((windows_group_update_kernel<T, WIN_BLEND>), grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, ebar, C, gt, tb, sched, st);
  else if (kind == WIN_DDPM)
    hipLaunchKernelGGL((windows_group_update_kernel<T, WIN_DDPM>), grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, ebar, C, gt, tb, sched, st);
  else
    hipLaunchKernelGGL((windows_group_update_kernel<T, WIN_DDIM>), grid, dim3(256), 0, s, x, eps_cl, noise, noise_step_stride, x_cl, ebar, C, gt, tb, sched, st);
  return hipGetLastError();
}
hipError_t launch_windows_group_update(int dt, int kind, float* x, const void* eps_cl, const float* noise, int64_t noise_step_stride, void* x_cl,
                                       float* ebar, int C, WinGroupTables gt, StepTables tb, const DdimStep* sched, const int* st, hipStream_t s) {
  if (kind != WIN_BLEND && kind != WIN_DDPM && kind != WIN_DDIM) return hipErrorInvalidValue;
  if (!win_group_tables_ok(gt) || !eps_cl || C <= 0 || (kind == WIN_DDIM && !sched)) return hipErrorInvalidValue;
  if (kind == WIN_BLEND ? !ebar : (!x || !x_cl || !st)) return hipErrorInvalidValue;
  if (dt == DT_F32) return launch_windows_group_update_t<float>(kind, x, eps_cl, noise, noise_step_stride, x_cl, ebar, C, gt, tb, sched, st, s);
  return launch_windows_group_update_t<__bf16>(kind, x, eps_cl, noise, noise_step_stride, x_cl, ebar, C, gt, tb, sched, st, s);
}

// Kind WIN_DPM ("DPM-Solver++ windows"): the DPM-Solver++(2M) update of dpm_update_kernel on the recordings' states
// with ONE history block x0_prev [C][Ltot_r] per recording, packed like x, from the blend of windows_group_update_kernel -- same tile
// table, same cover / weight / start tables, same blend (w * eps in fp32, window order, the first term assigned), same stores into x
// and into the row of every covering window of x_cl.  The history is loaded only where the entry says has_prev (and is not the last)
// and written on every iteration but the last; an entry without has_prev never reads it, so it is never cleared.  Nothing is drawn.
// Load order: as above; the history's load depends on the table row (has_prev), so it follows st -> row and is issued in front of the
// row -> coefficient-table loads and of everything that consumes them.
template <typename T>
__global__ __launch_bounds__(256) void windows_group_dpm_update_kernel(float* x, const void* eps_cl, float* x0_prev, void* x_cl, int C,
                                                                       WinGroupTables gt, StepTables tb, const DpmStep* sched, const int* st) {
  __shared__ float tile[32][33];
  const WinGroupTile te = gt.tile[blockIdx.x];
  const WinGroupRec rc = gt.rec[te.rec];
  const int c0 = blockIdx.y * 32, l0 = te.l0;
  const int Ltot = rc.Ltot, Lw = gt.Lw, w0 = rc.w0;
  const size_t xo = (size_t)C * rc.off;
  const int* cover = gt.cover + rc.cover_off;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  int cov[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int g = l0 + ty + ii * 8;
    cov[ii] = g < Ltot ? cover[g] : 0;
  }
  float ev[4], xin[4], pv[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int g = l0 + i, c = c0 + tx;
    const int first = w0 + (cov[ii] & 255), n = cov[ii] >> 8;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j < n && c < C) {
        const int k = first + j, l = g - gt.start[k];
        const float we = gt.weight[(size_t)k * Lw + l] * dld<T>(eps_cl, ((size_t)k * Lw + l) * C + c);
        acc = j == 0 ? we : acc + we;
      }
    ev[ii] = acc;
    const int cc = c0 + i, ll = l0 + tx;
    xin[ii] = (cc < C && ll < Ltot) ? x[xo + (size_t)cc * Ltot + ll] : 0.f;
  }
  const DpmStep sp = sched[st[1]];
  const bool hist = !sp.last && sp.has_prev;   // (uniform over the grid) the only case in which the history is read
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int cc = c0 + ty + ii * 8, ll = l0 + tx;
    pv[ii] = (hist && cc < C && ll < Ltot) ? x0_prev[xo + (size_t)cc * Ltot + ll] : 0.f;
  }
  const float recip = tb.sqrt_recip_alphas_cumprod[sp.t], recipm1 = tb.sqrt_recipm1_alphas_cumprod[sp.t];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = ev[ii];
  __syncthreads();
  float newv[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int c = c0 + i, g = l0 + tx;
    newv[ii] = 0.f;
    if (c < C && g < Ltot) {
      const size_t idx = xo + (size_t)c * Ltot + g;
      const float x0 = clipped_x0(recip, recipm1, xin[ii], tile[tx][i]);
      float v = x0;
      if (!sp.last) {
        v = sp.a * xin[ii] + sp.b0 * x0;
        if (hist) v += sp.b1 * pv[ii];
        x0_prev[idx] = x0;
      }
      x[idx] = v;
      newv[ii] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = newv[ii];   // tile[c][g]
  __syncthreads();
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int g = l0 + i, c = c0 + tx;
    const int first = w0 + (cov[ii] & 255), n = cov[ii] >> 8;
    const float v = tile[tx][i];
#pragma unroll
    for (int jj = 0; jj < 3; ++jj)
      if (jj < n && c < C) {
        const int k = first + jj, l = g - gt.start[k];
        dst<T>(x_cl, ((size_t)k * Lw + l) * C + c, v);
      }
  }
}

hipError_t launch_windows_group_dpm_update(int dt, float* x, const void* eps_cl, float* x0_prev, void* x_cl, int C, WinGroupTables gt, StepTables tb,
                                           const DpmStep* sched, const int* st, hipStream_t s) {
  if (!win_group_tables_ok(gt)) return hipErrorInvalidValue;
  if (!x || !eps_cl || !x0_prev || !x_cl || !sched || !st || C <= 0) return hipErrorInvalidValue;
  dim3 grid(gt.n_tiles, (C + 31) / 32, 1);
  if (dt == DT_F32) hipLaunchKernelGGL(windows_group_dpm_update_kernel<float>, grid, dim3(256), 0, s, x, eps_cl, x0_prev, x_cl, C, gt, tb, sched, st);
  else hipLaunchKernelGGL(windows_group_dpm_update_kernel<__bf16>, grid, dim3(256), 0, s, x, eps_cl, x0_prev, x_cl, C, gt, tb, sched, st);
  return hipGetLastError();
}

// the windows' slices of a packed fp32 sequence as the items of a channels-last batch (the to_cl_kernel tiling): window k reads the
// block of ITS recording r = wrec[k] -- [C][Ltot_r / div] at C * (off_r / div) floats -- from start[k] / div: y[k][l][c] = x_r[c][start[k] / div + l]
// (div = up for the raw condition: its blocks are [Cc][Ftot_r] at Cc * off_r / up)
template <typename T>
__global__ __launch_bounds__(256) void windows_group_gather_kernel(const float* x, void* y, int C, int Lw, WinGroupTables gt, int div) {
  __shared__ float tile[32][33];
  const int k = blockIdx.z, c0 = blockIdx.y * 32, l0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const WinGroupRec rc = gt.rec[gt.wrec[k]];
  const int Lr = rc.Ltot / div, s0 = gt.start[k] / div;
  const float* xr = x + (size_t)C * (rc.off / div);
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, l = l0 + tx;
    tile[i][tx] = (c < C && l < Lw && s0 + l < Lr) ? xr[(size_t)c * Lr + s0 + l] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int l = l0 + i, c = c0 + tx;
    if (l < Lw && c < C) dst<T>(y, ((size_t)k * Lw + l) * C + c, tile[tx][i]);
  }
}
// y [W][Lw][C] dt <- the windows' slices of the packed x; Lw: the frames of a window of THIS sequence (the group's Lw / div)
hipError_t launch_windows_group_gather(int dt, const float* x, void* y, int W, int C, int Lw, WinGroupTables gt, int div, hipStream_t s) {
  if (W <= 0 || Lw <= 0 || C <= 0 || div < 1 || !x || !y || !win_group_tables_ok(gt)) return hipErrorInvalidValue;
  dim3 grid((Lw + 31) / 32, (C + 31) / 32, W);
  if (dt == DT_F32) hipLaunchKernelGGL(windows_group_gather_kernel<float>, grid, dim3(256), 0, s, x, y, C, Lw, gt, div);
  else hipLaunchKernelGGL(windows_group_gather_kernel<__bf16>, grid, dim3(256), 0, s, x, y, C, Lw, gt, div);
  return hipGetLastError();
}

// the recordings' Philox keys written on the stream (kernel arguments carry them, as launch_ddim_table_write's entries: no host buffer
// outlives the call, a captured step graph takes the keys from memory)
struct WinGroupKeys { uint64_t k[32]; };
__global__ void windows_group_keys_kernel(WinGroupRec* rec, WinGroupKeys keys, int R) {
  const int r = threadIdx.x;
  if (r < R) { rec[r].key_lo = (unsigned)keys.k[r]; rec[r].key_hi = (unsigned)(keys.k[r] >> 32); }
}
hipError_t launch_windows_group_keys(WinGroupRec* rec, const uint64_t* keys_host, int R, hipStream_t s) {
  if (!rec || R < 1 || R > 32) return hipErrorInvalidValue;
  WinGroupKeys ks{};
  for (int r = 0; r < R; ++r) ks.k[r] = keys_host ? keys_host[r] : 0;
  hipLaunchKernelGGL(windows_group_keys_kernel, dim3(1), dim3(32), 0, s, rec, ks, R);
  return hipGetLastError();
}

// the item keys of a seeded call's batch part written on the stream, as launch_windows_group_keys writes the recordings' (kernel arguments
// carry them: no host buffer outlives the call, a captured step graph takes the keys from memory)
constexpr int kItemKeyChunk = 32;
struct ItemKeyChunk { uint64_t k[kItemKeyChunk]; };
__global__ void item_keys_write_kernel(uint64_t* dst, ItemKeyChunk src, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = src.k[threadIdx.x];
}
hipError_t launch_item_keys_write(uint64_t* dst, const uint64_t* keys_host, int n, hipStream_t s) {
  if (!dst || !keys_host || n < 1) return hipErrorInvalidValue;
  for (int i0 = 0; i0 < n; i0 += kItemKeyChunk) {
    ItemKeyChunk ch{};
    const int m = std::min(kItemKeyChunk, n - i0);
    for (int i = 0; i < m; ++i) ch.k[i] = keys_host[i0 + i];
    hipLaunchKernelGGL(item_keys_write_kernel, dim3(1), dim3(kItemKeyChunk), 0, s, dst + i0, ch, m);
  }
  return hipGetLastError();
}

// the DPM schedule table written on the stream, as launch_ddim_table_write writes its table
struct DpmChunk { DpmStep e[kDdimChunk]; };
__global__ void dpm_table_write_kernel(DpmStep* dst, DpmChunk src, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = src.e[threadIdx.x];
}
hipError_t launch_dpm_table_write(DpmStep* dst, const DpmStep* src, int n, hipStream_t s) {
  for (int i0 = 0; i0 < n; i0 += kDdimChunk) {
    DpmChunk ch{};
    const int m = std::min(kDdimChunk, n - i0);
    for (int i = 0; i < m; ++i) ch.e[i] = src[i0 + i];
    hipLaunchKernelGGL(dpm_table_write_kernel, dim3(1), dim3(kDdimChunk), 0, s, dst + i0, ch, m);
  }
  return hipGetLastError();
}

// tl (optional): device-side timeline of the timed (graph-replayed, multi-stream) mode: constant-rate clock (100 MHz,
// s_memrealtime) at the begin and the end of every step of this batch part, slot = the step's iteration index
__global__ void step_advance_kernel(int* st, unsigned long long* tl) {
  if (tl) tl[2 * (st[1] & 2047) + 1] = wall_clock64();
  st[0] -= 1;
  st[1] += 1;
}
__global__ void step_set_kernel(int* st, int t, int j, unsigned key_lo, unsigned key_hi) {
  st[0] = t;
  st[1] = j;
  st[2] = (int)key_lo;
  st[3] = (int)key_hi;
}
// First kernel of a denoise step.  Workgroup 0 owns the part's step state: with `advance` it first moves on from the previous step
// (t - 1, iteration + 1: until round 5 a one-thread launch of its own behind p_sample_update; the timeline's end stamp of that step
// is taken here), counts the UNet-pass epoch up (st[4]: the XCD-team chains tag their tile flags with it, never cleared, never 0)
// and copies the timestep's (scale | shift) row (DDIM: of the timestep the schedule table holds for iteration j); every other workgroup clears the step's accumulator region (GroupNorm sums,
// split-K counters, k-max keys: until round 3 a memset node of its own): zero_n16 16-byte pieces starting at `zero`.
__global__ __launch_bounds__(1024) void step_begin_kernel(const float* table, int stride, int* st, float* cur,
                                                          unsigned long long* tl, uint4* zero, long long zero_n16, int advance,
                                                          const int* t_words, int t_stride) {
  constexpr int nthr = 1024;
  if (blockIdx.x == 0) {
    __shared__ int sh_t;
    if (threadIdx.x == 0) {
      int t = st[0], j = st[1];
      const int epoch = st[4];
      const unsigned long long now = tl ? wall_clock64() : 0ull;
      if (advance) {
        if (tl && j >= 0) tl[2 * (j & 2047) + 1] = now;
        t -= 1;
        j += 1;
        st[0] = t;
        st[1] = j;
      }
      if (t_words) {   // DDIM, DPM: the timestep of iteration j comes from the strided schedule (the `t` word of the table's entry j)
        t = t_words[(size_t)max(j, 0) * t_stride];
        st[0] = t;
      }
      if (tl) tl[2 * (j & 2047)] = now;
      st[4] = epoch + 1;
      sh_t = t;
    }
    __syncthreads();
    const float* row = table + (size_t)max(sh_t, 0) * stride;
    const int n4 = stride >> 2;
    if ((stride & 3) == 0 && n4 <= 8 * nthr) {   // eight 16-byte loads in flight per thread: one memory latency for a 100 KB row, not one per element
      const float4* r4 = reinterpret_cast<const float4*>(row);
      float4* c4 = reinterpret_cast<float4*>(cur);
      const int i0 = threadIdx.x;
      const float4 v0 = r4[min(i0, n4 - 1)], v1 = r4[min(i0 + nthr, n4 - 1)], v2 = r4[min(i0 + 2 * nthr, n4 - 1)], v3 = r4[min(i0 + 3 * nthr, n4 - 1)];
      const float4 v4 = r4[min(i0 + 4 * nthr, n4 - 1)], v5 = r4[min(i0 + 5 * nthr, n4 - 1)], v6 = r4[min(i0 + 6 * nthr, n4 - 1)], v7 = r4[min(i0 + 7 * nthr, n4 - 1)];
      if (i0 < n4) c4[i0] = v0;
      if (i0 + nthr < n4) c4[i0 + nthr] = v1;
      if (i0 + 2 * nthr < n4) c4[i0 + 2 * nthr] = v2;
      if (i0 + 3 * nthr < n4) c4[i0 + 3 * nthr] = v3;
      if (i0 + 4 * nthr < n4) c4[i0 + 4 * nthr] = v4;
      if (i0 + 5 * nthr < n4) c4[i0 + 5 * nthr] = v5;
      if (i0 + 6 * nthr < n4) c4[i0 + 6 * nthr] = v6;
      if (i0 + 7 * nthr < n4) c4[i0 + 7 * nthr] = v7;
    } else {
      for (int i = threadIdx.x; i < stride; i += nthr) cur[i] = row[i];
    }
    if (gridDim.x > 1) return;
  }
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const long long nb = gridDim.x > 1 ? gridDim.x - 1 : 1, bi = gridDim.x > 1 ? blockIdx.x - 1 : 0;
  for (long long i = bi * nthr + threadIdx.x; i < zero_n16; i += nb * nthr) zero[i] = z;
}
hipError_t launch_step_begin_sched(const float* table, int stride, int* st, float* cur, unsigned long long* tl, hipStream_t s, void* zero,
                                   size_t zero_bytes, int advance, const int* t_words, int t_stride_ints) {
  const long long n16 = (long long)((zero_bytes + 15) / 16);
  const long long want = n16 > 0 ? 1 + (n16 + 4095) / 4096 : 1;
  hipLaunchKernelGGL(step_begin_kernel, dim3((unsigned)std::min<long long>(256, want)), dim3(1024), 0, s, table, stride, st, cur, tl,
                     reinterpret_cast<uint4*>(zero), n16, advance, t_words, t_stride_ints);
  return hipGetLastError();
}
hipError_t launch_step_begin(const float* table, int stride, int* st, float* cur, unsigned long long* tl, hipStream_t s,
                             void* zero, size_t zero_bytes, int advance, const DdimStep* ddim) {
  return launch_step_begin_sched(table, stride, st, cur, tl, s, zero, zero_bytes, advance, ddim ? &ddim->t : nullptr,
                                 (int)(sizeof(DdimStep) / sizeof(int)));
}
// one workgroup that holds its CU slot for `us` microseconds of the 100 MHz wall clock (bounded): the stream-overlap calibration of ldc_api.cpp
__global__ void spin_us_kernel(unsigned us) {
  const unsigned long long t0 = wall_clock64();
  int guard = 0;
  while (wall_clock64() - t0 < (unsigned long long)us * 100ull && guard < (1 << 20)) ++guard;
}
hipError_t launch_spin_us(unsigned us, hipStream_t s) {
  hipLaunchKernelGGL(spin_us_kernel, dim3(1), dim3(64), 0, s, us);
  return hipGetLastError();
}
__global__ void clock_sample_kernel(unsigned long long* out) {
  out[0] = wall_clock64();
  out[1] = __builtin_amdgcn_s_memtime();
}
hipError_t launch_clock_sample(unsigned long long* out2, hipStream_t s) {
  hipLaunchKernelGGL(clock_sample_kernel, dim3(1), dim3(1), 0, s, out2);
  return hipGetLastError();
}
hipError_t launch_step_advance(int* st, unsigned long long* tl, hipStream_t s) {
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, st, tl);
  return hipGetLastError();
}
hipError_t launch_step_set(int* st, int t, int j, uint64_t noise_key, hipStream_t s) {
  hipLaunchKernelGGL(step_set_kernel, dim3(1), dim3(1), 0, s, st, t, j, (unsigned)noise_key, (unsigned)(noise_key >> 32));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// output normalisation: x /= std(x)+1e-8 (unbiased) ; x /= max|x|+1e-8     (sample.py:133-134)
// ws per slot: double sum, double sumsq, then float maxabs array after the doubles
// ---------------------------------------------------------------------------------------------
size_t output_normalise_ws_bytes(int B) { return (size_t)B * (2 * sizeof(double) + sizeof(float)) + 16; }

__global__ __launch_bounds__(256) void outnorm_reduce_kernel(const float* x, int64_t n_per_item, int per_item,
                                                             double* sums, float* maxabs, const int* lens, int lens_unit) {
  const int b = blockIdx.y;
  const int64_t n_valid = lens ? min(n_per_item, (int64_t)lens[b] * lens_unit) : n_per_item;   // ragged batch: the item's own samples
  double s = 0.0, ss = 0.0;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_valid; i += (int64_t)gridDim.x * 256) {
    const float v = x[(size_t)b * n_per_item + i];
    s += v; ss += (double)v * v; m = fmaxf(m, fabsf(v));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o); ss += __shfl_xor(ss, o); m = fmaxf(m, __shfl_xor(m, o));
  }
  __shared__ double rs[4], rss[4];
  __shared__ float rm[4];
  if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = s; rss[threadIdx.x >> 6] = ss; rm[threadIdx.x >> 6] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int slot = per_item ? b : 0;
    atomicAdd(&sums[2 * slot], rs[0] + rs[1] + rs[2] + rs[3]);
    atomicAdd(&sums[2 * slot + 1], rss[0] + rss[1] + rss[2] + rss[3]);
    atomicMax(reinterpret_cast<unsigned*>(maxabs) + slot, __float_as_uint(fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3]))));
  }
}

__global__ __launch_bounds__(256) void outnorm_apply_kernel(float* x, int64_t n_per_item, int per_item, int B,
                                                            const double* sums, const float* maxabs, const int* lens, int lens_unit) {
  const int b = blockIdx.y;
  const int slot = per_item ? b : 0;
  const int64_t n_valid = lens ? min(n_per_item, (int64_t)lens[b] * lens_unit) : n_per_item;
  const double n = per_item ? (double)n_valid : (double)n_per_item * B;
  const double mean = sums[2 * slot] / n;
  double var = (sums[2 * slot + 1] - n * mean * mean) / (n - 1.0);
  if (var < 0.0) var = 0.0;
  const float sd = (float)sqrt(var) + 1e-8f;
  const float mx = maxabs[slot] / sd + 1e-8f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_per_item; i += (int64_t)gridDim.x * 256) {
    const size_t idx = (size_t)b * n_per_item + i;
    x[idx] = i < n_valid ? (x[idx] / sd) / mx : 0.f;
  }
}

hipError_t launch_output_normalise(float* x, int B, int64_t n_per_item, int per_item, void* ws, hipStream_t s, const int* lens, int lens_unit) {
  if (lens && !per_item) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(ws, 0, output_normalise_ws_bytes(B), s);
  if (e != hipSuccess) return e;
  double* sums = reinterpret_cast<double*>(ws);
  float* maxabs = reinterpret_cast<float*>(sums + 2 * B);
  int bx = (int)std::min<int64_t>((n_per_item + 255) / 256, 64);
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(outnorm_reduce_kernel, dim3(bx, B), dim3(256), 0, s, x, n_per_item, per_item, sums, maxabs, lens, lens_unit);
  hipLaunchKernelGGL(outnorm_apply_kernel, dim3(bx, B), dim3(256), 0, s, x, n_per_item, per_item, B, sums, maxabs, lens, lens_unit);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Ragged batches: the padding rows of x [B][L][C] (rows l >= lens[b] >> shift) written as zero.  An item's padding is one contiguous
// byte range behind its valid rows, so the kernel only stores (16-byte pieces; nothing of the padding is read): grid (chunks, B).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_rows_kernel(uint4* x, int L, long long row16, const int* lens, int shift) {
  const int b = blockIdx.y;
  const int Lv = valid_rows(lens, shift, b, L);
  const long long lo = ((long long)b * L + Lv) * row16, hi = ((long long)b + 1) * L * row16;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  for (long long i = lo + (long long)blockIdx.x * 256 + threadIdx.x; i < hi; i += (long long)gridDim.x * 256) x[i] = z;
}
hipError_t launch_mask_rows(int dt, void* x, int B, int L, int C, const int* lens, int shift, hipStream_t s) {
  const size_t row_bytes = (size_t)C * dt_size(dt);
  if (!lens || row_bytes % 16 || (reinterpret_cast<uintptr_t>(x) & 15)) return hipErrorInvalidValue;
  const long long row16 = (long long)(row_bytes / 16);
  const int bx = (int)std::max<long long>(1, std::min<long long>(((long long)L * row16 + 255) / 256, 64));
  hipLaunchKernelGGL(mask_rows_kernel, dim3(bx, B), dim3(256), 0, s, reinterpret_cast<uint4*>(x), L, row16, lens, shift);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void mask_codes_kernel(int64_t* codes, int n_q, int B, int F, const int* flens) {
  const int64_t n = (int64_t)n_q * B * F;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int f = (int)(i % F), b = (int)((i / F) % B);
    if (f >= flens[b]) codes[i] = 0;
  }
}
hipError_t launch_mask_codes(int64_t* codes, int n_q, int B, int F, const int* flens, hipStream_t s) {
  const int64_t n = (int64_t)n_q * B * F;
  hipLaunchKernelGGL(mask_codes_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024))), dim3(256), 0, s, codes, n_q,
                     B, F, flens);
  return hipGetLastError();
}

// the lengths of a ragged batch written on the stream, as launch_ddim_table_write writes its table
constexpr int kLensChunk = 64;
struct LensChunk { int v[kLensChunk]; };
__global__ void lens_write_kernel(int* dst, LensChunk src, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = src.v[threadIdx.x];
}
hipError_t launch_lens_write(int* dst, const int* src, int n, hipStream_t s) {
  for (int i0 = 0; i0 < n; i0 += kLensChunk) {
    LensChunk ch{};
    const int m = std::min(kLensChunk, n - i0);
    for (int i = 0; i < m; ++i) ch.v[i] = src[i0 + i];
    hipLaunchKernelGGL(lens_write_kernel, dim3(1), dim3(kLensChunk), 0, s, dst + i0, ch, m);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Per-item step state (ItemState, ldc_kernels.h): the kernels of a per-item plan that read or move it.
// ---------------------------------------------------------------------------------------------
constexpr int kItemChunk = 32;
struct ItemChunk { ItemState v[kItemChunk]; };
__global__ void items_write_kernel(ItemState* dst, ItemChunk src, int n, int* lens, int* flens, int up) {
  const int i = threadIdx.x;
  if (i >= n) return;
  dst[i] = src.v[i];
  if (lens) lens[i] = src.v[i].len;
  if (flens) flens[i] = src.v[i].len / up;
}
hipError_t launch_items_write(ItemState* dst, const ItemState* src, int n, int* lens, int* flens, int up, hipStream_t s) {
  if (up < 1) return hipErrorInvalidValue;
  for (int i0 = 0; i0 < n; i0 += kItemChunk) {
    ItemChunk ch{};
    const int m = std::min(kItemChunk, n - i0);
    for (int i = 0; i < m; ++i) ch.v[i] = src[i0 + i];
    hipLaunchKernelGGL(items_write_kernel, dim3(1), dim3(kItemChunk), 0, s, dst + i0, ch, m, lens ? lens + i0 : nullptr,
                       flens ? flens + i0 : nullptr, up);
  }
  return hipGetLastError();
}

// step_begin_kernel for a per-item plan.  Workgroup 0 owns the items' states: active = remaining > 0, a running item moves on when asked to
// (t - 1, j + 1, one step less remaining: a slot stops behind t = 0 by itself; an item with a schedule takes t from entry j + 1 of it and
// stops behind its last entry), the part's epoch word is counted up once.  No row is
// copied: gn_apply reads the (scale | shift) row of each item's t from the table.  Every other workgroup clears the accumulator region.
__global__ __launch_bounds__(1024) void step_begin_items_kernel(ItemState* items, int B, int* st, uint4* zero, long long zero_n16, int advance) {
  constexpr int nthr = 1024;
  if (blockIdx.x == 0) {
    for (int b = threadIdx.x; b < B; b += nthr) {
      ItemState* it = items + b;
      const int run = it->remaining > 0;
      if (run && advance) {
        const SchedEntry* sc = it->sched;
        const int j = it->j + 1;
        it->t = sc ? sc[max(j, 0)].t : it->t - 1;   // DDIM, DPM: the timestep of iteration j of the item's own strided schedule
        it->j = j;
        it->remaining -= 1;
      }
      it->active = run;
    }
    if (threadIdx.x == 0) st[4] = st[4] + 1;
    if (gridDim.x > 1) return;
  }
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const long long nb = gridDim.x > 1 ? gridDim.x - 1 : 1, bi = gridDim.x > 1 ? blockIdx.x - 1 : 0;
  for (long long i = bi * nthr + threadIdx.x; i < zero_n16; i += nb * nthr) zero[i] = z;
}
hipError_t launch_step_begin_items(ItemState* items, int B, int* st, void* zero, size_t zero_bytes, int advance, hipStream_t s) {
  const long long n16 = (long long)((zero_bytes + 15) / 16);
  const long long want = n16 > 0 ? 1 + (n16 + 4095) / 4096 : 1;
  hipLaunchKernelGGL(step_begin_items_kernel, dim3((unsigned)std::min<long long>(256, want)), dim3(1024), 0, s, items, B, st,
                     reinterpret_cast<uint4*>(zero), n16, advance);
  return hipGetLastError();
}

// p_sample_update_kernel with everything about the step read from the item's record.  Same 32 x 32 tiling; the item's state is [C][len]
// on its own length, so a tile behind the item's end (and every tile of an idle item) leaves before it touches memory.  The sampler is
// the item's too: a record without a schedule takes p_sample's arithmetic, one with a schedule ddim_update_kernel's (ITEM_DDIM) or
// dpm_update_kernel's (ITEM_DPM) with the coefficients of sched[j].  The branch is uniform over the workgroup (one item per
// blockIdx.z), so one launch serves any mix of the three.  x0_prev is the DPM items' history, item b's [C][len] block at the stride
// of x: only a DPM item touches it, and it loads it only on an iteration that has a predecessor and is not the last.
template <typename T>
__global__ __launch_bounds__(256) void p_sample_update_items_kernel(float* x, int64_t x_item_stride, const void* eps_cl, void* x_cl, int C,
                                                                    int Lmax, StepTables tb, const ItemState* items, int n_t,
                                                                    float* x0_prev) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, l0 = blockIdx.x * 32;
  const ItemState it = items[b];
  const int L = min(it.len, Lmax);
  const bool sched = it.sched != nullptr;
  const bool dpm = sched && it.kind == ITEM_DPM, ddim = sched && !dpm;
  // (uniform over the workgroup) idle: neither x, x_cl nor the history is stored, neither the tape nor the schedule is dereferenced.
  // A DPM record in a launch without a history is not run either
  if (!it.active || l0 >= L || (dpm && !x0_prev)) return;
  float* xb = x + (size_t)b * x_item_stride;
  float* hb = x0_prev + (dpm ? (size_t)b * x_item_stride : 0);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  // the tensor loads need the record only: issue them before the dependent chain schedule entry -> coefficient tables.  So does the
  // history's: behind step_begin_items_kernel, "has a predecessor" is j >= 1 and "last" is remaining == 0 (what the table's has_prev and
  // last say).  Iteration 0 and the last iteration do not load it: whatever an earlier item left in the slot reaches no value
  const int j = it.j;
  const bool hist = dpm && j >= 1 && it.remaining > 0;
  float ev[4], xin[4], pv[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int l = l0 + i, c = c0 + tx;
    ev[ii] = (l < L && c < C) ? dld<T>(eps_cl, ((size_t)b * Lmax + l) * C + c) : 0.f;
    const int cc = c0 + i, ll = l0 + tx;
    xin[ii] = (cc < C && ll < L) ? xb[(size_t)cc * L + ll] : 0.f;
    pv[ii] = (hist && cc < C && ll < L) ? hb[(size_t)cc * L + ll] : 0.f;
  }
  SchedEntry se;
  se.ddim = DdimStep{};
  if (sched) se = it.sched[min(max(j, 0), n_t - 1)];   // (the pool's arena row holds n_t entries)
  const DdimStep& sp = se.ddim;   // (read only under ddim)
  const DpmStep& dp = se.dpm;     // (read only under dpm)
  const int t = min(max(sched ? se.t : it.t, 0), n_t - 1);
  const float recip = tb.sqrt_recip_alphas_cumprod[t], recipm1 = tb.sqrt_recipm1_alphas_cumprod[t];
  float c1 = 0.f, c2 = 0.f, sigma = ddim ? sp.sigma : 0.f;
  if (!sched) {
    c1 = tb.posterior_mean_coef1[t];
    c2 = tb.posterior_mean_coef2[t];
    sigma = expf(0.5f * tb.posterior_log_variance_clipped[t]);
  }
  // noise is read or drawn only here: DDPM at t > 0, DDIM on an iteration that is not the last and has sigma > 0, DPM never (neither
  // its tape pointer nor its key is used)
  const bool draw = dpm ? false : ddim ? (!sp.last && sp.sigma > 0.f) : t > 0;
  const uint64_t seed = ((uint64_t)it.key_hi << 32) | (uint64_t)it.key_lo;
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = ev[ii];
  __syncthreads();
  float newv[4];
  // one Philox block per thread at the index of its first element IN THE ITEM ALONE (c * len + l): what ldc_denoise / ldc_ddim_sample draw
  // for it at B = 1
  float zz[4] = {0.f, 0.f, 0.f, 0.f};
  if (draw && !it.noise) philox_normal4(seed, (unsigned)j, (uint64_t)(c0 + ty) * L + l0 + tx, zz);
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int i = ty + ii * 8;
    const int c = c0 + i, l = l0 + tx;
    newv[ii] = 0.f;
    if (c < C && l < L) {
      const size_t idx = (size_t)c * L + l;
      const float xv = xin[ii];
      const float e = tile[tx][i];
      float x0 = recip * xv - recipm1 * e;
      x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
      float v;
      if (dpm) {   // dpm_update_kernel: the table's last / has_prev choose the coefficients, pv was loaded where the record agrees
        v = x0;
        if (!dp.last) {
          v = dp.a * xv + dp.b0 * x0;
          if (dp.has_prev) v += dp.b1 * pv[ii];
          hb[idx] = x0;
        }
      } else if (ddim) {
        v = x0;
        if (!sp.last) {
          v = x0 * sp.sqrt_an + sp.c * e;
          if (draw) v += sigma * (it.noise ? it.noise[(size_t)j * C * L + idx] : zz[ii]);
        }
      } else {
        v = c1 * x0 + c2 * xv;
        if (draw) v += sigma * (it.noise ? it.noise[(size_t)j * C * L + idx] : zz[ii]);
      }
      xb[idx] = v;
      newv[ii] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) tile[ty + ii * 8][tx] = newv[ii];   // tile[c][l]
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int l = l0 + i, c = c0 + tx;
    if (l < L && c < C) dst<T>(x_cl, ((size_t)b * Lmax + l) * C + c, tile[tx][i]);
  }
}
hipError_t launch_p_sample_update_items(int dt, float* x, int64_t x_item_stride, const void* eps_cl, void* x_cl, int B, int C, int Lmax,
                                        StepTables tb, const ItemState* items, int T, float* x0_prev, hipStream_t s) {
  dim3 grid((Lmax + 31) / 32, (C + 31) / 32, B);
  if (dt == DT_F32)
    hipLaunchKernelGGL(p_sample_update_items_kernel<float>, grid, dim3(256), 0, s, x, x_item_stride, eps_cl, x_cl, C, Lmax, tb, items, T,
                       x0_prev);
  else
    hipLaunchKernelGGL(p_sample_update_items_kernel<__bf16>, grid, dim3(256), 0, s, x, x_item_stride, eps_cl, x_cl, C, Lmax, tb, items, T,
                       x0_prev);
  return hipGetLastError();
}

}  // namespace ldc

// ---------------------------------------------------------------------------------------------
// Front end: torchaudio.functional.resample (sinc_interp_hann), the call at srcs/sample.py:84.  Polyphase form: output sample
// i * new + p = sum_k kernel[p][k] * padded[i * orig + k] with the [new][2 width + orig] filter bank built on the host in
// float64 (torchaudio 0.13 _get_sinc_resample_kernel) -- one thread per output sample, HBM/L2-bound streaming.
// ---------------------------------------------------------------------------------------------
namespace ldc {
__global__ __launch_bounds__(256) void resample_kernel(const float* wav, int64_t T, const float* bank, int orig, int nnew, int width,
                                                       int K, int64_t target, float* out) {
  const int c = blockIdx.y;
  const float* x = wav + (size_t)c * T;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < target; j += (int64_t)gridDim.x * 256) {
    const int64_t i = j / nnew;
    const int p = (int)(j - i * nnew);
    const float* kr = bank + (size_t)p * K;
    const int64_t s0 = i * orig - width;          // index into the unpadded signal of tap 0
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
      const int64_t s = s0 + k;
      if (s >= 0 && s < T) acc = fmaf(x[s], kr[k], acc);
    }
    out[(size_t)c * target + j] = acc;
  }
}
hipError_t launch_resample(const float* wav, int C, int64_t T, const float* bank, int orig, int nnew, int width, int64_t target, float* out,
                           hipStream_t s) {
  if (target <= 0 || C <= 0) return hipSuccess;
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)std::min<int64_t>((target + 255) / 256, 2048), C), dim3(256), 0, s, wav, T, bank, orig,
                     nnew, width, 2 * width + orig, target, out);
  return hipGetLastError();
}
}  // namespace ldc
