// conv_fast.inc -- (compiled once per dtype by conv_fast_bf16.hip / conv_fast_f32.hip)
// the pipelined conv-GEMM used by every UNet conv (zero padding, no prologue
// activation, plain Conv1d incl. stride 2, nearest-x2-upsample folding and two concatenated inputs).
//
// Same implicit-GEMM tiling as conv_gemm.hip (BM output positions x BN output channels per
// workgroup, 32x32 MFMA sub-tiles), restructured around the CDNA4 memory path:
//   * HBM/L2 -> LDS copies are LDS-DMA (`global_load_lds_dwordx4`: 64 lanes x 16 B land lane-linear in
//     LDS, no VGPR round trip), issued through inline asm so that hipcc's waitcnt pass neither waits
//     for them nor drains them before the ds_reads of the stage being consumed (with the builtin it
//     inserts `s_waitcnt vmcnt(0)` in front of the first ds_read and serialises copy and math);
//   * an S-stage LDS ring (S compile-time, the unit loop is unrolled by S so every LDS address is a
//     precomputed register + immediate): the copies of units u+1..u+S-1 are in flight while unit u is
//     multiplied, released with a counted `s_waitcnt vmcnt(N)` + one barrier per unit;
//   * a pipeline UNIT = NS sub-steps of (one tap, one 64-byte channel chunk): 3 taps x 1 chunk for k=3,
//     4 x 1 for k=4 / k=7 (two groups), 1 tap x 2 chunks for 1x1 convs;
//   * LDS-DMA cannot pad rows, so bank conflicts are avoided with an XOR swizzle of the 16-byte slot
//     index, slot' = slot ^ ((row >> 2) & 3), applied to the per-lane SOURCE address and again to the
//     ds_read address (16 rows distinct mod 16 -> 16 distinct bank slots; SQ_LDS_BANK_CONFLICT < 1 %);
//   * everything that does not depend on the channel chunk -- the per-tap input-row gather incl. padding
//     / stride / upsample, the swizzled fragment addresses for every ring stage, the per-lane DMA source
//     rows -- is computed once per workgroup: the first version spent 11 VALU + 9 SALU instructions per
//     MFMA on address arithmetic (rocprofv3 SQ_INSTS_*), which, not LDS or L2, was what bounded it.
// Round 4 -- what a launch can carry besides the conv (DESIGN.md section 4, profiles/r04_fusion_experiments.md):
//   * the GroupNorm APPLY of a ResnetBlock's Block in the epilogue (ConvKArgs::gn_part, conv_device.h: epilogue_gn_fused) with the
//     item-major tile order its in-launch statistics exchange needs;
//   * a folded 1x1 conv over the same input (template RF, ConvLayer::wtaps: res_conv beside block1's conv);
//   * a folded PreNorm LayerNorm (ConvKArgs::ln_s: row statistics in the prologue, applied to the accumulators);
//   * per-launch device stamps of the timed mode (ConvKArgs::kst).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "conv_device.h"

#ifndef LDC_FAST_W8
#define LDC_FAST_W8 0
#endif
#ifndef LDC_FAST_FP8
#define LDC_FAST_FP8 0
#endif

namespace ldc {
namespace LDC_FAST_NS {

// LDC_FAST_W8: the weights are OCP fp8 (e4m3) with one fp32 scale per output channel (BASELINE config 5): a weight row of
// a chunk is 32 bytes instead of 64, so the weight slabs -- 60 % of what a workgroup copies per unit -- cost half the
// LDS-DMA traffic; a B fragment is one ds_read_b64 expanded to bf16 in registers (every e4m3 value is exact in bf16), the
// MFMA stays v_mfma_f32_32x32x16_bf16 and the scale is applied with the bias in the epilogue.  The four 8-byte slots
// of a weight row are pre-permuted in the packed image (slot ^ ((n >> 3) & 3)): the copy stays linear, the reads are
// conflict-free.
static constexpr bool kW8 = LDC_FAST_W8 != 0;
// LDC_FAST_FP8: BOTH operands are OCP fp8 e4m3 (T is a one-byte tag type): a 64-byte LDS row holds 64 channels, a pipeline unit
// twice the reduction depth of the bf16 kernel for the same bytes, and the MFMA is the block-scaled
// v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales (E8M0 127) -- the only fp8 form that runs at twice the bf16 rate on gfx950
// (the unscaled fp8 MFMAs run at the bf16 rate).  A lane's operand is 32 bytes = the two 16-byte slots (2 kh, 2 kh + 1) of its
// row; both operands use the same byte -> k assignment, so the order inside a chunk is irrelevant.  Outputs are bf16, the
// per-output-channel weight scale is applied with the bias in the epilogue.
static constexpr bool kFp8 = LDC_FAST_FP8 != 0;
struct fp8_tag { unsigned char v; };
typedef int i32x8 __attribute__((ext_vector_type(8)));
static constexpr int kRowBytesB = kW8 ? 32 : 64;

__device__ __forceinline__ uint4 expand_fp8x8(const uint2& v) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, false);
  const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, false);
  const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, true);
  return make_uint4(hw_bf16x2(a[0], a[1]), hw_bf16x2(b[0], b[1]), hw_bf16x2(c[0], c[1]), hw_bf16x2(d[0], d[1]));
}

// counted wait on the VMEM counter
__device__ __forceinline__ void wait_vmcnt(int n) {
  switch (n) {
#define LDC_W(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    LDC_W(0) LDC_W(1) LDC_W(2) LDC_W(3) LDC_W(4) LDC_W(5) LDC_W(6) LDC_W(7) LDC_W(8) LDC_W(9) LDC_W(10) LDC_W(11)
    LDC_W(12) LDC_W(13) LDC_W(14) LDC_W(15) LDC_W(16) LDC_W(17) LDC_W(18) LDC_W(19) LDC_W(20) LDC_W(21) LDC_W(22)
    LDC_W(23) LDC_W(24) LDC_W(25) LDC_W(26) LDC_W(27) LDC_W(28) LDC_W(29) LDC_W(30) LDC_W(31) LDC_W(32) LDC_W(33)
    LDC_W(34) LDC_W(35) LDC_W(36) LDC_W(37) LDC_W(38) LDC_W(39) LDC_W(40) LDC_W(41) LDC_W(42) LDC_W(43) LDC_W(44)
    LDC_W(45) LDC_W(46) LDC_W(47) LDC_W(48)
#undef LDC_W
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// one LDS-DMA: lane l's 16 bytes at (base + voff) land at LDS byte address lds_addr + 16*l.  M0 carries the
// wave-uniform LDS address and is saved/restored (hipcc does not model M0 inside an asm statement).
__device__ __forceinline__ void lds_dma16(const char* base, unsigned voff, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(base), "s"(lds_addr)
               : "memory");
}

// RF: a 1x1 conv over the same input is folded in (ConvLayer::wtaps, ResnetBlock.res_conv beside block1.proj): one more weight
// slab per unit, multiplied with the centre-tap window already in LDS into a second accumulator set (k = 3, one chunk per unit)
template <typename T, int WM, int WN, int TM, int TN, int TG, int KC, int S, int NA, bool RF>
__device__ __forceinline__ void conv_fast_body(const ConvKArgs& a, const FastGeom& gm, const unsigned bid) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32, NW = WM * WN, NS = TG * KC;
  static_assert(!RF || (TG == 3 && KC == 1 && !kW8 && !kFp8), "the folded 1x1 conv rides on a k = 3 bf16 / f32 unit");
  constexpr int TGL = RF ? TG + 1 : TG;   // weight slabs per chunk of a unit
  constexpr int NSB = TGL * KC;
  using TO = typename std::conditional<kFp8, __bf16, T>::type;   // output / residual element type
  static_assert(S == 2, "the window planes hold only the sweep groups that are copied: that needs the S == 2 consumer (vmcnt(0))");
  constexpr int BKE = kRowBytes / (int)sizeof(T);
  constexpr int NB = (NSB * BN * kRowBytesB + NW * 1024 - 1) / (NW * 1024);   // LDS-DMA sweeps per wave: weight slabs of a unit
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void* lptr_t;
  const unsigned lds_base = (unsigned)(size_t)(lptr_t)smem;

  const int tid = ldc_tid(), lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int M = a.B * a.L_rows;
  unsigned long long t_start = 0, t_pro = 0, t_loop = 0, t_tab = 0, t_dma = 0;
  if (gm.stamps) t_start = __builtin_amdgcn_s_memtime();
  unsigned long long* const kst_slot = kst_begin(a, tid, bid);   // timed-mode stamps
  if (gm.debug & 8) return;   // tuning aid: launch + boundary cost of this grid
  // XCD-aware tile order: workgroup h runs on XCD h % 8 (observed dispatch rule, used for speed only), so give
  // every XCD a contiguous run of tiles, N-tile fastest: workgroups sharing an input window hit the same L2.
  int m0, n0, sk_k, sk_tile;
  {
    const int ntiles = gm.ntiles;   // split-K: slice ks of every tile lives at blockIdx ks * ntiles + tile
    sk_k = a.ksplit > 1 ? (int)fdiv(bid, gm.d_ntiles) : 0;
    sk_tile = (int)bid - sk_k * ntiles;
    if (gm.sk_xcd) {
      // Split-K by 2 or 4 (the 1024-channel levels): workgroup bid runs on XCD bid & 7, and that XCD takes ONE K slice (its low bits)
      // and the N tiles of one residue (its high bits) for every M tile -- an eighth of the weights as before, but a half / a quarter
      // of the input channels instead of all of them (the windows were fetched by all eight L2s: 19 of a launch's 47 MB at L = 75).
      // N tile fastest inside an M tile: an item's tiles stay adjacent in dispatch order (fused GroupNorm apply).
      const int lg = a.ksplit == 4 ? 2 : 1;
      const int x = (int)bid & 7, q = (int)bid >> 3;
      sk_k = x & (a.ksplit - 1);
      const int mt = (int)fdiv((unsigned)q, gm.d_skper);
      const int per = gm.ntn >> (3 - lg);
      const int nt = ((q - mt * per) << (3 - lg)) + (x >> lg);
      m0 = mt * BM;
      n0 = nt * BN;
      sk_tile = mt * gm.ntn + nt;
    }
    const int h = sk_tile;
    const int xcd = h & 7, slot = h >> 3;
    const int q = ntiles >> 3, r = ntiles & 7;
    const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    if (gm.sk_xcd) {
      // (m0, n0 set above)
    } else if (gm.item_major) {
      // Fused GroupNorm apply: a tile waits for every tile of its item(s), so the DISPATCH order must walk the items -- with
      // the per-XCD runs above, eight far-apart items would be in flight and their waiting tiles could hold every slot of the
      // chip while the tiles they wait for have none (two chains share the CUs).  Groups of 8 consecutive M-tiles, all their
      // N-tiles: inside a group workgroup h takes M-tile (h & 7), so the N-tiles of one window still meet in one XCD's L2,
      // and at most one or two items are incomplete at any time.
      // Weight-heavy layers (item_major == 2; N tiles a multiple of 8): workgroup h of a group takes the N tiles congruent to
      // h & 7 instead, for all eight M tiles of the group -- every XCD then streams an eighth of the weights rather than all of
      // them (with the M mapping the 1024-channel levels fetched 5-6x their unique bytes: profiles/r04_conv_pmc_classes.md).
      const int G = gm.ntn << 3;
      const int grp = (int)fdiv((unsigned)h, gm.d_grp);
      const int hl = h - grp * G;
      int mt, nt;
      if (gm.item_major == 3 && grp < (gm.ntm >> 3)) {
        // 4 x 2 arrangement of the XCDs over (N residue mod 4, M-tile parity) for layers whose windows and weights are of similar size:
        // an XCD streams a quarter of the weights and half of the group's windows (8 x 1: an eighth and ALL windows -- 45 instead of
        // 32 MB per launch on 1024 -> 1024 at L = 150)
        const int x = hl & 7, slot = hl >> 3;
        const int ml = (int)fdiv((unsigned)slot, gm.d_skper);   // (d_skper = ntn / 4 here)
        mt = (grp << 3) + (ml << 1) + (x >> 2);
        nt = (x & 3) + ((slot - ml * (gm.ntn >> 2)) << 2);
      } else if (gm.item_major >= 2 && grp < (gm.ntm >> 3)) {
        const int slot = hl >> 3, per = gm.ntn >> 3;          // slot in [0, ntn): (M tile of the group, which of this XCD's N tiles)
        const int ml = (int)fdiv((unsigned)slot, gm.d_per);
        mt = (grp << 3) + ml;
        nt = (hl & 7) + ((slot - ml * per) << 3);
      } else if (grp < (gm.ntm >> 3)) {
        mt = (grp << 3) + (hl & 7);
        nt = hl >> 3;
      } else {
        const int rem = gm.ntm & 7;
        nt = (int)fdiv((unsigned)hl, gm.d_rem);
        mt = (grp << 3) + hl - nt * rem;
      }
      m0 = mt * BM;
      n0 = nt * BN;
    } else if (gm.m_fastest) {   // weight-heavy layer: an XCD keeps few N-tiles, so every weight slab lives in ONE L2
      const int nt = (int)fdiv((unsigned)t, gm.d_ntm);
      n0 = nt * BN;
      m0 = (t - nt * gm.ntm) * BM;
    } else {
      const int mt = (int)fdiv((unsigned)t, gm.d_ntn);
      m0 = mt * BM;
      n0 = (t - mt * gm.ntn) * BN;
    }
  }

  int R_lo, R_hi;
  tile_window(a, m0, BM, M, R_lo, R_hi);
  const int nrows = min(R_hi - R_lo + 1, gm.a_rows);
  const int plane_bytes = (gm.a_rows + 1) * kRowBytes;
  const int zero_off = gm.a_rows * kRowBytes;
  const int b_off = KC * plane_bytes;
  // per-lane DMA sources, chunk-independent part
  unsigned dma_row[NA], dma_s16[NA];   // window: flat input row and swizzled 16-byte slot offset
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int p = (i * NW + wave) * 64 + lane;
    int r = p >> 2;
    dma_s16[i] = (unsigned)(((p & 3) ^ ((r >> 2) & 3)) << 4);
    if (r >= nrows) r = 0;
    dma_row[i] = (unsigned)(R_lo + r);
  }
  unsigned dma_b[NB];                      // weights: byte offset inside the (chunk group 0, tap group 0) slab set
  const unsigned slab_bytes = (unsigned)a.n_pad * kRowBytesB;       // one tap of one chunk
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int p = (i * NW + wave) * 64 + lane;
    if (kW8) {
      const int off = p * 16;                 // linear copy: the image is pre-permuted
      int q = off / (BN * kRowBytesB);
      const int rem = off - q * (BN * kRowBytesB);
      if (q >= NS) q = 0;
      const int kc = q / TG, t = q - kc * TG;
      dma_b[i] = (unsigned)(kc * a.wtaps + t) * slab_bytes + (unsigned)n0 * kRowBytesB + (unsigned)rem;
    } else {
      const int rb = p >> 2;
      const int s = (p & 3) ^ ((rb >> 2) & 3);
      int q = rb / BN;
      const int j = rb - q * BN;
      if (q >= NSB) q = 0;
      const int kc = q / TGL, t = q - kc * TGL;
      dma_b[i] = (unsigned)(kc * a.wtaps + t) * slab_bytes + (unsigned)(n0 + j) * kRowBytes + (unsigned)(s << 4);
    }
  }

  if (gm.stamps) t_tab = __builtin_amdgcn_s_memtime();
  const int nchunks = (a.C1 + a.C2) / BKE;
  const int nunits_all = (nchunks / KC) * gm.ngroups;
  // this workgroup's slice of the pipeline units: [u_begin, nunits)
  const int u_begin = a.ksplit > 1 ? (int)fdiv((unsigned)(nunits_all * sk_k), gm.d_ksplit) : 0;
  const int nunits = a.ksplit > 1 ? (int)fdiv((unsigned)(nunits_all * (sk_k + 1)), gm.d_ksplit) : nunits_all;
  constexpr int per_unit = KC * NA + NB;     // LDS-DMA instructions per wave per unit (wave-uniform)

  // producer cursor: (chunk group, tap group) of the next unit to copy
  int lu_c0 = (u_begin >> (gm.ngroups - 1)) * KC, lu_g = u_begin & (gm.ngroups - 1);   // ngroups is 1 or 2
  auto load_unit = [&](int st) {
    const unsigned stage_lds = lds_base + (unsigned)(st * gm.stage_bytes) + (unsigned)(wave * 1024);
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      const int c = lu_c0 + kc;
      const char* src;
      unsigned ldb, cofb;
      if (c * BKE < a.C1) {
        src = a.x1; ldb = a.C1 * (unsigned)sizeof(T); cofb = (unsigned)c * kRowBytes;
      } else {
        src = a.x2; ldb = a.C2 * (unsigned)sizeof(T); cofb = (unsigned)(c * BKE - a.C1) * (unsigned)sizeof(T);
      }
      // a sweep instruction covers 16 window rows: the ones wholly behind the window's last row are not issued (a 128-position
      // k=3 tile needs 130 rows = 9 of the 12 instructions of its three sweeps).  Only legal with S == 2, whose consumer
      // waits for vmcnt(0) rather than counting instructions.
#pragma unroll
      for (int i = 0; i < NA; ++i)
        if (S != 2 || (i * NW + wave) * 16 < nrows) {
          lds_dma16(src, dma_row[i] * ldb + dma_s16[i] + cofb, stage_lds + (unsigned)(kc * plane_bytes + i * NW * 1024));
        }
    }
    const int tg0 = lu_g * TG;
    const unsigned unit_b = (unsigned)(lu_c0 * a.wtaps + tg0) * slab_bytes;
    if (gm.ngroups == 1) {
#pragma unroll
      for (int i = 0; i < NB; ++i) lds_dma16(a.w, dma_b[i] + unit_b, stage_lds + (unsigned)(b_off + i * NW * 1024));
    } else {
      // k=7: the last tap group is short; its unused slab is pointed at a valid one
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int p = (i * NW + wave) * 64 + lane;
        int q = (p * 16) / (BN * kRowBytesB);
        if (q >= NS) q = 0;
        const int t = q % TG;
        const unsigned off = (tg0 + t >= a.taps) ? dma_b[i] - (unsigned)t * slab_bytes : dma_b[i];
        lds_dma16(a.w, off + unit_b, stage_lds + (unsigned)(b_off + i * NW * 1024));
      }
    }
    if (++lu_g == gm.ngroups) { lu_g = 0; lu_c0 += KC; }
  };

#pragma unroll
  for (int p = 0; p < S - 1; ++p)
    if (u_begin + p < nunits) load_unit(p);
  if (gm.stamps) t_dma = __builtin_amdgcn_s_memtime();
  if constexpr (!kFp8) {
    if (a.ln_s) ln_row_stats<T, BM, NW * 64>(a, reinterpret_cast<float*>(smem + gm.ln_off), m0, M, tid);   // folded PreNorm LayerNorm (conv_device.h)
  }
  // everything below is independent of the copies just issued: it runs under their latency
  // zero rows (one behind every plane of every stage)
  for (int i = tid; i < S * KC * 16; i += NW * 64) {
    const int st = i / (KC * 16), rem = i - st * (KC * 16);
    reinterpret_cast<unsigned*>(smem + (size_t)st * gm.stage_bytes + (rem >> 4) * plane_bytes + zero_off)[rem & 15] = 0u;
  }

  const int kh = lane >> 5;
  int row_b[TM], row_l[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + (wm * TM + i) * 32 + (lane & 31);
    if (m < M) {
      row_b[i] = (int)fdiv((unsigned)m, a.lrows_div);
      row_l[i] = m - row_b[i] * a.L_rows;
    } else {
      row_b[i] = -1;
      row_l[i] = 0;
    }
  }
  // LDS byte addresses of this lane's fragments for every ring stage / plane (wave-uniform offsets folded in)
  unsigned a_ad[S][KC][TM][TG][2];
  auto calc_arows = [&](int g) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        int off0 = zero_off, off1 = zero_off;
        const int tap = g * TG + t;
        if (row_b[i] >= 0 && tap < a.taps) {
          const int gr = gather_row(a, row_b[i], row_l[i], tap * a.dil);
          if (gr >= 0) {
            const int row = gr - R_lo;
            const int sw = (row >> 2) & 3;
            off0 = row * kRowBytes + (((kFp8 ? 2 * kh : kh) ^ sw) << 4);
            off1 = row * kRowBytes + (((kFp8 ? 2 * kh + 1 : 2 + kh) ^ sw) << 4);
          }
        }
#pragma unroll
        for (int ss = 0; ss < S; ++ss)
#pragma unroll
          for (int kc = 0; kc < KC; ++kc) {
            a_ad[ss][kc][i][t][0] = (unsigned)(ss * gm.stage_bytes + kc * plane_bytes + off0);
            a_ad[ss][kc][i][t][1] = (unsigned)(ss * gm.stage_bytes + kc * plane_bytes + off1);
          }
      }
  };
  calc_arows(0);
  unsigned b_ad[S][TN][2];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int rb = wn * TN * 32 + j * 32 + (lane & 31);
    const int sw = (rb >> 2) & 3;
#pragma unroll
    for (int ss = 0; ss < S; ++ss) {
      if (kW8) {
        const int s8 = (rb >> 3) & 3;
        b_ad[ss][j][0] = (unsigned)(ss * gm.stage_bytes + b_off + rb * kRowBytesB + ((kh ^ s8) << 3));
        b_ad[ss][j][1] = (unsigned)(ss * gm.stage_bytes + b_off + rb * kRowBytesB + (((2 + kh) ^ s8) << 3));
      } else {
        b_ad[ss][j][0] = (unsigned)(ss * gm.stage_bytes + b_off + rb * kRowBytes + (((kFp8 ? 2 * kh : kh) ^ sw) << 4));
        b_ad[ss][j][1] = (unsigned)(ss * gm.stage_bytes + b_off + rb * kRowBytes + (((kFp8 ? 2 * kh + 1 : 2 + kh) ^ sw) << 4));
      }
    }
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  f32x16 acc2[RF ? TM : 1][RF ? TN : 1];   // folded 1x1 conv
  if constexpr (RF) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[i][j][r] = 0.0f;
  }

  int cu_g = u_begin & (gm.ngroups - 1);   // consumer cursor: tap group of the unit being multiplied
  if (gm.stamps) t_pro = __builtin_amdgcn_s_memtime();
  for (int u0 = u_begin; u0 < ((gm.debug & 16) ? min(nunits, u_begin + 1) : nunits); u0 += S) {
#pragma unroll
    for (int ss = 0; ss < S; ++ss) {
      const int u = u0 + ss;
      if (u >= nunits) break;
      // my copies of unit u have landed once at most min(S-2, units after u) later units are outstanding
      if (S == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else wait_vmcnt(min(S - 2, nunits - 1 - u) * per_unit);
      __syncthreads();   // every wave's part of unit u is visible; every wave is done with unit u-1 -> its stage is free
      if (u + S - 1 < nunits && !(gm.debug & 1)) load_unit((ss + S - 1) % S);
      if (gm.ngroups > 1) calc_arows(cu_g);
      // straight-line MFMA chain: no run-time branch may sit between the fragment reads and the MFMAs of a unit
      // (a conditional `continue` here made hipcc park the 32-64 accumulator registers elsewhere around every
      // (tap, k-step) group: 48 v_mov + s_nop per 4 MFMAs, ~95 instead of ~35 cycles per MFMA).  The short last tap
      // group of k = 7 multiplies the zero row instead of being skipped (calc_arows points tap >= taps there).
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        const int kc = q / TG, t = q % TG;
        if constexpr (kFp8) {
          // one (tap, 64-channel chunk): each operand fragment is the lane's two 16-byte slots, ONE scaled MFMA of depth 64
          uint4 af[TM][2], bfr[TN][2];
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) af[i][h2] = *reinterpret_cast<const uint4*>(smem + a_ad[ss][kc][i][t][h2]);
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) bfr[j][h2] = *reinterpret_cast<const uint4*>(smem + b_ad[ss][j][h2] + q * (BN * kRowBytes));
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              i32x8 va, vb;
              __builtin_memcpy(&va, &af[i][0], 32);
              __builtin_memcpy(&vb, &bfr[j][0], 32);
              acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, vb, acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
            }
        } else {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          uint4 af[TM], bfr[TN];
#pragma unroll
          for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const uint4*>(smem + a_ad[ss][kc][i][t][ks]);
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            if (kW8) bfr[j] = expand_fp8x8(*reinterpret_cast<const uint2*>(smem + b_ad[ss][j][ks] + q * (BN * kRowBytesB)));
            else bfr[j] = *reinterpret_cast<const uint4*>(smem + b_ad[ss][j][ks] + q * (BN * kRowBytes));
          }
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) mfma_step<T>(acc[i][j], af[i], bfr[j]);
        }
        }
      }
      if constexpr (RF) {   // the folded 1x1 conv: centre-tap window rows (tap 1 of the k = 3 conv) x the unit's fourth slab
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          uint4 af[TM], bfr[TN];
#pragma unroll
          for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const uint4*>(smem + a_ad[ss][0][i][1][ks]);
#pragma unroll
          for (int j = 0; j < TN; ++j) bfr[j] = *reinterpret_cast<const uint4*>(smem + b_ad[ss][j][ks] + NS * (BN * kRowBytes));
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) mfma_step<T>(acc2[i][j], af[i], bfr[j]);
        }
      }
      if (++cu_g == gm.ngroups) cu_g = 0;
    }
  }

  if (gm.stamps) t_loop = __builtin_amdgcn_s_memtime();
  __syncthreads();   // every wave has consumed the last ring stage: LDS is free for the output transpose
  if (a.ksplit > 1) {   // park the partial tile; the last slice to arrive sums all slices and carries on into the epilogue
    if (!splitk_park_and_sum<TM, TN, NW>(a, acc, smem, sk_tile, sk_k, wave, lane, tid)) return;
  }
  if constexpr (!kFp8) {
    if (a.ln_s) ln_apply<TM, TN>(a, acc, reinterpret_cast<const float*>(smem + gm.ln_off), wm * TM * 32, n0 + wn * TN * 32, lane);
  }
  {
    constexpr int WREG = TM * 32 * (TN * 32 * (int)sizeof(TO) + 16);
    constexpr int WREG32 = TM * 32 * (TN * 32 * 4 + 16);   // fused GroupNorm apply with a residual stages fp32 rows
    const int wreg = (a.residual || (a.gn_part && (a.gn_out & 1))) ? WREG32 : WREG;   // (a residual is added to fp32-staged rows, fused GroupNorm apply or not)
    if constexpr (RF) {
      if (!(gm.debug & 4)) epilogue_rows_second<TO, TM, TN>(a, acc2, smem + (size_t)wave * wreg, m0 + wm * TM * 32, n0 + wn * TN * 32, M);
    }
    if (!(gm.debug & 4)) epilogue_rows_dispatch<TO, TM, TN>(a, acc, smem + (size_t)wave * wreg, m0 + wm * TM * 32, n0 + wn * TN * 32, M, m0, BM, WM, wm, 0);
    else if (acc[0][0][0] == 12345.678f) a.y[0] = 1;   // tuning aid: keep the accumulators live, store nothing
  }
  kst_end(kst_slot, tid, bid, gm.grid);
  if (gm.stamps) stamp_phases(gm.stamps, tid, bid, t_start, t_pro, t_loop, t_tab, t_dma);
}


#include "conv_lean.inc"

template <typename T, int WM, int WN, int TM, int TN, int TG, int KC, int S, int NA, bool RF>
__global__ __launch_bounds__(WM* WN * 64, 2) void conv_fast_kernel(const ConvKArgs a, const FastGeom gm) {
  conv_fast_body<T, WM, WN, TM, TN, TG, KC, S, NA, RF>(a, gm, blockIdx.x);
}

template <typename T, int WM, int WN, int TM, int TN, int TG, int KC, int S, int NA, bool RF = false>
static hipError_t launch_fast_cfg(const ConvKArgs& a_in, const FastGeom& gm_in, int M, hipStream_t s) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  ConvKArgs a = a_in;
  FastGeom gm = gm_in;
  const int tiles = ((M + BM - 1) / BM) * (a.n_pad / BN);
  const int tiles_dec = tiles;
  {   // split-K for few-tile, long-K layers (the L = 75 / 150 levels)
    static const ConvTune kDefault;
    const ConvTune& tn = a.tune ? *a.tune : kDefault;
    const int nunits = (((a.C1 + a.C2) * (int)sizeof(T)) / kRowBytes / KC) * gm.ngroups;
    int ks = 1;
    if (tn.splitk >= 1 && gm.ngroups == 1 && tiles_dec <= tn.sk_tiles && !gm.stamps) {
      if (tn.splitk == 1) ks = nunits >= tn.sk_u3 ? 3 : (nunits >= tn.sk_u2 ? 2 : 1);
      else if (nunits >= 12 * tn.splitk) ks = tn.splitk;
    }
    if (a.sk_need) {   // dry run: report the workspace this launch would want (and the tile height)
      *a.sk_need = ks > 1 ? (long long)tiles * ks * BM * BN : 0;
      if (a.bm_out) { a.bm_out[0] = BM; a.bm_out[1] = WM; a.bm_out[2] = ks; a.bm_out[3] = BN; }
      return hipSuccess;
    }
    // fused GroupNorm apply: a tile may straddle three items, not four, and a 32-column block must lie inside one group (the
    // planner asked for the tile shape first and sized gn_part with it)
    if (a.gn_part && (2 * a.L_rows < BM || a.gn_cpg % 32 || a.n % 32 || a.gn_mslots < (a.L_rows + BM - 1) / BM + 1)) {
      if (getenv("LDC_VERBOSE")) fprintf(stderr, "[ldc] fused GroupNorm apply refused: BM %d L_rows %d cpg %d n %d mslots %d\n", BM, a.L_rows, a.gn_cpg, a.n, a.gn_mslots);
      return hipErrorInvalidValue;
    }
    if (!a.sk_part || !a.sk_count || tiles > a.sk_count_cap || (long long)tiles * ks * BM * BN > a.sk_part_cap) ks = 1;
    if (a.ln_s) ks = 1;   // (1x1 convs of <= 32 units never split anyway)
    a.ksplit = ks;
    if (RF && ks > 1) { if (getenv("LDC_VERBOSE")) fprintf(stderr, "[ldc] folded conv with split-K %d refused (tiles %d)\n", ks, tiles); return hipErrorInvalidValue; }   // the second accumulator set is not parked: the planner folds only where K is not split
    a.ksplit = ks;
  }
  dim3 grid(tiles * a.ksplit);
  gm.grid = tiles * a.ksplit;
  gm.ntiles = tiles; gm.ntn = a.n_pad / BN; gm.ntm = tiles / gm.ntn;
  gm.d_ntiles = make_fastdiv((unsigned)tiles); gm.d_ntn = make_fastdiv((unsigned)gm.ntn); gm.d_ntm = make_fastdiv((unsigned)gm.ntm);
  gm.d_ksplit = make_fastdiv((unsigned)a.ksplit);
  {
    const bool sk_xcd_on = true;
    const int nl = a.ksplit == 4 ? 2 : (a.ksplit == 2 ? 4 : 0);   // N tiles per group of eight workgroups
    gm.sk_xcd = (sk_xcd_on && nl && gm.ntn % nl == 0) ? 1 : 0;
    gm.d_skper = make_fastdiv((unsigned)std::max(1, nl ? gm.ntn / nl : 1));
  }
  gm.item_major = a.gn_part ? ((gm.m_fastest && gm.ntn % 8 == 0) ? 2 : 1) : 0;   // m_fastest: the weights are the larger operand (LDC_FAST_ENTRY)
  if (gm.item_major == 2 && !gm.sk_xcd) {
    // bytes the eight L2s fetch per launch: weights x (XCDs along M) + windows x (XCDs along N)
    const bool grid42_on = true;
    const double w_bytes = (double)(a.C1 + a.C2) * a.wtaps * a.n_pad * sizeof(T);
    const double a_bytes = (double)a.B * a.L_in * (a.C1 + a.C2) * sizeof(T);
    if (grid42_on && gm.ntn % 4 == 0 && 2 * w_bytes + 4 * a_bytes < w_bytes + 8 * a_bytes) {
      gm.item_major = 3;
      gm.d_skper = make_fastdiv((unsigned)std::max(1, gm.ntn / 4));
    }
  }
  gm.d_grp = make_fastdiv((unsigned)(gm.ntn * 8)); gm.d_rem = make_fastdiv((unsigned)std::max(1, gm.ntm & 7));
  gm.d_per = make_fastdiv((unsigned)std::max(1, gm.ntn >> 3));
  auto kern = conv_fast_kernel<T, WM, WN, TM, TN, TG, KC, S, NA, RF>;
  static bool lds_opt_in = false;
  if (!lds_opt_in) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    lds_opt_in = true;
  }
  using TO = typename std::conditional<kFp8, __bf16, T>::type;
  const size_t epi_bytes = (size_t)WM * WN * TM * 32 * (TN * 32 * ((a.residual || (a.gn_part && (a.gn_out & 1))) ? 4 : sizeof(TO)) + 16);
  const size_t lds_pad = 0;
  gm.ln_off = 0;
  size_t ln_bytes = 0;
  if (a.ln_s) {
    if (a.taps != 1 || a.C2 != 0 || a.stride != 1 || a.ups != 0 || a.ksplit != 1 || kFp8) return hipErrorInvalidValue;   // (the planner folds only the attention blocks' to_qkv)
    gm.ln_off = (int)((std::max((size_t)S * gm.stage_bytes, epi_bytes) + 15) / 16 * 16);
    ln_bytes = (size_t)gm.ln_off + (size_t)BM * 8 - std::max((size_t)S * gm.stage_bytes, epi_bytes);
  }
  if constexpr (WM == 2 && WN == 2 && TN == 1 && S == 2 && (TM == 1 || TM == 2)) {
    // round 6: the same launch on the instruction-diet kernel where its shapes allow (conv_lean.inc; ConvTune::lean = 0 keeps this kernel)
    bool lean_launched = false;
    const hipError_t le = launch_lean<T, TM, TG, KC, RF>(a, gm, M, s, &lean_launched);
    if (le != hipSuccess || lean_launched) return le;
  }
  if (a.qkv_ctx_ws) return hipErrorInvalidValue;   // (conv_fast_kernel has no context epilogue)
  hipLaunchKernelGGL(kern, grid, dim3(WM * WN * 64), std::max((size_t)S * gm.stage_bytes, epi_bytes) + ln_bytes + lds_pad, s, a, gm);
  return hipGetLastError();
}

// Ring depth of THIS kernel stays 2.  A deeper ring was tried on it three times in rounds 2 - 5 (S = 4, three units in flight, one
// workgroup per CU: slower at every grid size) and lost each time, with three things against it that are this kernel's, not the idea's:
// a copy cost ~40 instructions here (save M0 / set / copy / restore + address rebuild), so the loop was bound by copy ISSUE; the
// deeper ring kept s_waitcnt vmcnt(0) + __syncthreads() in front of every unit, which drains the extra unit again; and it was applied
// to every grid, so the dense launches lost a co-resident workgroup.  conv_lean_kernel (one instruction per copy) has a three-stage
// ring with a counted copy wait and a bare barrier for the sparse grids on 64-row tiles (conv_lean.inc, round 9): 20 - 25 % off those
// launches, 3.3 % off a decode -- and still a loss on the 128-row tiles, for the third reason (profiles/r09_ring3.md).
// Round 10: those tiles keep their third workgroup with a third stage for the WINDOW alone (conv_lean.inc, LEAN_RING_W: three window
// planes, two slab sets, 51.2 KB on the k = 3 128 x 64 tile): 1.0 - 1.5 % off a decode (profiles/r10_ring_window.md).
template <typename T, int TG, int KC, int NA, bool RF = false>
static hipError_t launch_fast_bn(int bn, const ConvKArgs& a, const FastGeom& gm, int M, hipStream_t s) {
  // Weights straight into VGPRs (each wave loading its own B fragments with global_load_dwordx4, only the activation
  // window staged by LDS-DMA) was built and measured: parity-clean but 10-50 % slower on every k=1/3/4 layer (k3
  // 256->256 @1200: 14.5 -> 16.7 us, k3 1024->1024 @75: 19.2 -> 28.7 us, end to end 173.6 -> 194.8 ms): a fragment
  // load touches 32 rows x 16 B of 64-byte rows and the two waves of a tile column fetch the same fragments.
  // Deeper rings of conv_fast_kernel, measured twice for the 64-wide tiles (before and after the MFMA chain was made branch-free):
  // S = 3 is 5-30 % slower, S = 4 ~85 % slower (k3 1024->1024 at L = 75: 19.8 / 22.0 / 37.3 us; end to end 167.8 ->
  // 177.5 ms with S = 3 on the 128 x 64 tiles): the extra stage costs a co-resident workgroup per CU -- see above for what else
  // those tries had against them, and profiles/r09_ring3.md for the lean kernel's three-stage ring, which the launches of these
  // tiles now take where it costs no workgroup (ConvTune::ring3_tiles, ring3_wgs).
  if (bn == 3) return hipErrorInvalidValue;
  if (bn == 0) return launch_fast_cfg<T, 2, 2, 1, 1, TG, KC, 2, NA, RF>(a, gm, M, s);   // 64 x 64 tile for small grids
  if (bn == 1) return launch_fast_cfg<T, 2, 2, 2, 1, TG, KC, 2, NA, RF>(a, gm, M, s);   // 128 x 64 tile for medium grids
  if (bn == 128) return hipErrorInvalidValue;   // (128 x 128 tiles: faster in isolation, slower with two parts in flight since round 3; removed in round 6)
  if (bn == 64) return launch_fast_cfg<T, 2, 2, 2, 1, TG, KC, 2, NA, RF>(a, gm, M, s);
  // 128 x 32 tiles (N not a multiple of 64: the UNet's final 1x1 conv); the entry point sends other kernel sizes of such layers to the generic kernel
  if constexpr (TG == 1 && !RF) return launch_fast_cfg<T, 4, 1, 1, 1, TG, KC, 2, NA, RF>(a, gm, M, s);
  else return hipErrorInvalidValue;
}

}  // namespace LDC_FAST_NS

hipError_t LDC_FAST_ENTRY(const ConvLayer& ly, const ConvKArgs& a_in, int M, int span_rows, hipStream_t s, bool* launched) {
  *launched = false;
  using namespace LDC_FAST_NS;
  FastGeom gm;
  ConvKArgs a = a_in;
  const int bn = ly.bn;
  const int bke = kRowBytes / (int)dt_size(ly.dt);
  const int nchunks = (ly.cin1 + ly.cin2) / bke;
  // 32-bit byte offsets inside the kernel
  if ((double)a.B * a.L_in * std::max(a.C1, a.C2) * dt_size(ly.dt) >= 2.0e9) return hipSuccess;
  if ((double)nchunks * ly.taps * ly.n_pad * LDC_FAST_NS::kRowBytesB >= 2.0e9) return hipSuccess;
  static const ConvTune kDefault;
  const ConvTune& tn = a.tune ? *a.tune : kDefault;
  const int tiles128 = ((M + 127) / 128) * (ly.n_pad / 128);
  // force_tile (self-check / tuning aid): 0 = 64 x 64, 1 = 128 x 64 for the layers whose N is a multiple of 128
  int ft = bn == 128 ? tn.force_tile : -1;
  if (ft == 3) ft = -1;   // (256 x 64 tiles: built in round 5, measured slower, removed in round 6)
  const bool small = ft >= 0 ? ft == 0 : (bn == 128 && tiles128 <= tn.small_max);
  int TG, KC = 1;
  if (ly.taps == 1) {
    TG = 1;
    const bool kc2 = nchunks % 2 == 0 && (ly.cin1 / bke) % 2 == 0;
    KC = kc2 ? 2 : 1;
  } else if (ly.taps == 3) {
    TG = 3;
  } else if (ly.taps == 4 || ly.taps == 7 || ly.taps == 8) {
    TG = 4;
  } else {
    return hipSuccess;   // other kernel sizes: generic path
  }
  if (bn == 32 && TG != 1) return hipSuccess;   // (narrow layers other than 1x1: generic path)
  const int quantum = 16 * 4;
  gm.ngroups = (ly.taps + TG - 1) / TG;
  // Larger grids use 128 x 64 tiles (medium): in isolation 128 x 128 is faster (half the weight-slab copies per
  // output), but the decode runs two batch parts on two streams and 41 KB of ring per workgroup lets three
  // workgroups of different kernels/phases share a CU (+2.4 % end to end, A/B on one box, round 3).  The 128 x 128
  // instantiations were removed in round 6 (a quarter of the library's code, chosen by no default).
  // Small grids (the L = 75 / 150 levels: 80-300 tiles of 128 x 128 for 256 CUs) are latency-bound with one
  // workgroup per CU at best: 64 x 64 tiles give 4x the workgroups, each with a quarter of the serial K loop.
  const bool medium = ft >= 0 ? ft >= 1 : (bn == 128 && !small);
  int tile_n = medium ? 64 : bn;
  if (small) {
    tile_n = 64;
    const int u_last = (a.L_rows - 1) * ly.stride + (ly.taps - 1) * ly.dil - ly.pad_left;
    const int leftover = std::max(0, ((a.L_in << ly.ups) - 1 - u_last)) >> ly.ups;
    span_rows = ((63 * ly.stride + (ly.taps - 1) * ly.dil) >> ly.ups) + 1 + ly.ups + ((64 + a.L_rows - 1) / a.L_rows + 1) * leftover;
  }
  gm.a_rows = (span_rows + quantum - 1) / quantum * quantum;
  const bool rf = a.y2 != nullptr;   // folded 1x1 conv: one more weight slab per unit
  if (rf && (TG != 3 || KC != 1 || LDC_FAST_NS::kW8 || LDC_FAST_NS::kFp8 || a.wtaps != 4)) return hipErrorInvalidValue;
  gm.b_rows = ((TG + (rf ? 1 : 0)) * KC * tile_n * LDC_FAST_NS::kRowBytesB / kRowBytes + quantum - 1) / quantum * quantum;   // in 64-byte rows
  gm.stage_bytes = (KC * (gm.a_rows + 1) + gm.b_rows) * kRowBytes;
  if ((size_t)gm.stage_bytes * 2 > 160 * 1024) return hipSuccess;
  // window sweeps per wave are a template parameter: 2 or 3 (stride 1 / upsample), 5 (k=4 stride 2)
  int na = gm.a_rows / quantum;
  if (TG == 4 && na <= 3) na = 3;
  else if (TG == 4 && na <= 5) na = 5;
  else if (TG != 4 && na <= 2) na = 2;
  else if (TG != 4 && na <= 3) na = 3;
  else return hipSuccess;
  // LDS planes hold whole 16-row sweep groups of the window, not whole sweeps: the groups behind the window's last row are
  // never copied (load_unit), so they need no room either (a 128-position k=3 tile: 144 + 1 rows per plane instead of 192 + 1)
  gm.a_rows = std::min(na * quantum, (span_rows + 15) / 16 * 16);
  gm.stage_bytes = (KC * (gm.a_rows + 1) + gm.b_rows) * kRowBytes;
  if ((size_t)gm.stage_bytes * 2 > 160 * 1024) return hipSuccess;
  gm.debug = tn.debug;
  gm.stamps = g_conv_stamps;
  {
    const int mf = tn.m_fastest;
    const double w_bytes = (double)nchunks * ly.taps * ly.n_pad * LDC_FAST_NS::kRowBytesB;
    const double a_bytes = (double)a.B * a.L_in * (a.C1 + a.C2) * dt_size(ly.dt);
    gm.m_fastest = (mf == 2 || (mf == 1 && w_bytes > a_bytes)) ? 1 : 0;
  }
  a.tg = TG;
  *launched = true;
  const int cfg = small ? 0 : (medium ? 1 : bn);
#if !LDC_FAST_W8 && !LDC_FAST_FP8
  if (rf) return na == 2 ? launch_fast_bn<LDC_FAST_T, 3, 1, 2, true>(cfg, a, gm, M, s) : launch_fast_bn<LDC_FAST_T, 3, 1, 3, true>(cfg, a, gm, M, s);
#endif
#define LDC_FAST(TT)                                                                                   \
  if (TG == 3) return na == 2 ? launch_fast_bn<TT, 3, 1, 2>(cfg, a, gm, M, s) : launch_fast_bn<TT, 3, 1, 3>(cfg, a, gm, M, s); \
  if (TG == 4) return na == 3 ? launch_fast_bn<TT, 4, 1, 3>(cfg, a, gm, M, s) : launch_fast_bn<TT, 4, 1, 5>(cfg, a, gm, M, s); \
  if (KC == 2) return na == 2 ? launch_fast_bn<TT, 1, 2, 2>(cfg, a, gm, M, s) : launch_fast_bn<TT, 1, 2, 3>(cfg, a, gm, M, s); \
  return na == 2 ? launch_fast_bn<TT, 1, 1, 2>(cfg, a, gm, M, s) : launch_fast_bn<TT, 1, 1, 3>(cfg, a, gm, M, s);
  LDC_FAST(LDC_FAST_T)
#undef LDC_FAST
}

// How many workgroups of the kernels this engine's fused-GroupNorm convs land on fit one CU (occupancy query with the launch's dynamic
// LDS; the worst of the k = 3 instantiations).  The planner's residency gate (ldc_api.cpp: few_tiles) is built on it instead of a constant.
int LDC_FAST_RESIDENCY() {
  using namespace LDC_FAST_NS;
  int worst = 1 << 30;
#if !LDC_FAST_W8 && !LDC_FAST_FP8
  for (const int n : {lean_gn_wgs_per_cu<LDC_FAST_T, 1, false, LEAN_RING_2>(), lean_gn_wgs_per_cu<LDC_FAST_T, 2, false, LEAN_RING_2>(),
                      lean_gn_wgs_per_cu<LDC_FAST_T, 1, true, LEAN_RING_2>(), lean_gn_wgs_per_cu<LDC_FAST_T, 2, true, LEAN_RING_2>()})
    worst = std::min(worst, n);
#else
  const size_t b_rows = (3 * 64 * LDC_FAST_NS::kRowBytesB / kRowBytes + 63) / 64 * 64;
  worst = std::min(worst, lean_ask_wgs(reinterpret_cast<const void*>(conv_fast_kernel<LDC_FAST_T, 2, 2, 1, 1, 3, 1, 2, 2, false>), 2 * (80 + 1 + b_rows) * kRowBytes));
  worst = std::min(worst, lean_ask_wgs(reinterpret_cast<const void*>(conv_fast_kernel<LDC_FAST_T, 2, 2, 2, 1, 3, 1, 2, 3, false>), 2 * (144 + 1 + b_rows) * kRowBytes));
#endif
  return worst == (1 << 30) ? 0 : worst;
}

}  // namespace ldc
