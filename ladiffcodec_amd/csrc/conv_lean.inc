// conv_lean.inc -- the pipelined conv-GEMM on an instruction diet (included by conv_fast.inc; instantiated by the bf16 and f32 engines).
//
// Same arithmetic as conv_fast_body (same LDS window / weight slabs / XOR swizzle, same MFMA order per accumulator, same epilogues:
// the results are bit-identical), a third of the instructions:
//   * the tile of a workgroup -- (m0, n0, split-K slice, window rows, unit range), in the XCD-aware dispatch order -- is ONE 32-byte
//     scalar load from a table the host builds per launch geometry (lean_tile_table);
//   * an LDS-DMA copy is ONE instruction: a wave's copies of a plane are contiguous in LDS, so M0 is written once per run and the
//     copies address their 1 KiB pieces through the instruction's immediate offset (the immediate is added to the LDS address AND to
//     the global address: the per-lane source offsets are pre-biased once per tile; tools/glds_probe.hip); the channel-chunk advance is
//     two scalar adds on the base pointer per unit;
//   * LDS layout constants (plane, stage, slab offsets) are compile-time: fragment addresses are TM x TG x 2 registers + immediates;
//   * the weight slabs of a unit lie [16-column group][slab][16 rows] in LDS, so that a wave's slab copies are contiguous too;
//   * epilogue kind, folded second conv, folded LayerNorm, split-K and the ring are template parameters chosen by the launcher: an
//     instantiation carries only its own path.
// Unit kinds (LeanShape): LEAN_K3 (3 taps x 1 chunk, optionally with the folded 1x1 conv's fourth slab), LEAN_K1 (1 tap x 2 chunks),
// LEAN_K1_LN (the same with the folded PreNorm LayerNorm), and for the bf16 engine (ConvTune::lean_all) LEAN_K4S2 (4 taps, stride 2: a
// plane of 2 BM + 2 rows, up to five pieces per wave, copied as two runs) and LEAN_K7 (a chunk makes TWO units, taps 0-3 | 4-6 and
// the zero row against a valid slab, as conv_fast_body multiplies it: the two stages are the two tap groups).
// Ring kinds (LeanRing, LeanRingTraits): two stages; three full stages; three window planes + two slab sets.  launch_lean chooses per
// launch: the deeper rings go to the sparse grids where they cost the CU no co-resident workgroup (ConvTune::ring3_*).
// The launcher keeps conv_fast_kernel for fp8 weights / activations, the 4 x 1-wave tiles, post-activations, the unfused GroupNorm
// statistics, k = 4 / 7 in f32 and k = 8.
// Measurements: profiles/r06_conv_issue.md (the diet), r07_kernel_stats.md (k = 4 / 7), r09_ring3.md, r10_ring_window.md (the rings),
// r11_lean_one_ring.md (the one ring loop: resource table before / after).

struct LeanTile { int m0, n0, sk_k, sk_tile, R_lo, nrows, u_begin, u_end; };   // one per workgroup, dispatch order
struct LeanGeom {
  const LeanTile* tiles;
  unsigned long long* stamps;   // tuning aid (LDC_CONV_STAMPS): per workgroup {start, prologue done, loop done, end, tables, first copies} s_memtime
  int debug;                    // ConvTune::debug bits (1 no copies after the prologue, 4 no output stores, 8 return at once, 16 one unit only)
  int ln_off;                   // folded LayerNorm: LDS byte offset of the tile's (mean, rstd) table
  int grid;
};

// unit kinds: 3 taps x 1 chunk | 1 tap x 2 chunks | the same with the folded PreNorm | 4 taps x 1 chunk, stride 2 | (4 + 3) taps: two units per chunk
enum { LEAN_K3 = 0, LEAN_K1 = 1, LEAN_K1_LN = 2, LEAN_K4S2 = 3, LEAN_K7 = 4 };
enum { LEAN_EPI_PLAIN = 0, LEAN_EPI_RES = 1, LEAN_EPI_GN = 2, LEAN_EPI_GN_RES = 3, LEAN_EPI_QKV = 4 };

template <int TM_, int KIND_, bool RF_>
struct LeanShape {
  static constexpr int TM = TM_, KIND = KIND_;
  static constexpr bool RF = RF_;
  static constexpr bool K3 = KIND == LEAN_K3, K4 = KIND == LEAN_K4S2, K7 = KIND == LEAN_K7;
  static constexpr bool TAPS = K3 || K4 || K7;                             // a unit is the tap slabs of ONE chunk
  static constexpr int TG = K3 ? 3 : (TAPS ? 4 : 1), KC = TAPS ? 1 : 2, NS = TG * KC, NSB = NS + (RF ? 1 : 0);
  static constexpr int NTAP = K7 ? 8 : TG;                                 // fragment address sets per row block (k = 7: both tap groups; tap 7 is the zero row)
  static constexpr int BM = TM * 64, BN = 64;
  // window rows a plane holds (stride 1: BM + taps - 1, stride 2: 2 BM + 2, rounded up to 16)
  static constexpr int PLANE_ROWS = K4 ? (TM == 2 ? 272 : 144) : (TAPS ? (TM == 2 ? 144 : 80) : BM);
  static constexpr int NAW = (PLANE_ROWS / 16 + 3) / 4;                    // 1 KiB window pieces per wave and plane (wave w: pieces w NAW ..)
  static constexpr int NAW0 = NAW > 3 ? 3 : NAW, NAW1 = NAW - NAW0;        // ... copied as one or two runs
  static constexpr int PLANE_BYTES = PLANE_ROWS * kRowBytes + kRowBytes;   // + the zero row behind the plane
  static constexpr int ZERO_OFF = PLANE_ROWS * kRowBytes;
  static constexpr int B_OFF = KC * PLANE_BYTES;
  static constexpr int SLAB_BYTES = NSB * BN * kRowBytes;                  // the slabs of one unit
  static constexpr int STAGE_BYTES = B_OFF + SLAB_BYTES;
  static_assert(NAW >= 1 && NAW <= 5 && NAW1 <= 2 && NSB >= 2 && NSB <= 4, "runs of at most four copies per M0 write (13-bit immediate)");
};

// The ring of a kernel: how many units are in flight under the unit being multiplied, and what the wait in front of a unit leaves out.
//   LEAN_RING_2: two stages.  One unit in flight, every unit drains the copy counter (vmcnt(0)) in front of a __syncthreads() -- right
//     where three workgroups share a CU and cover each other's waits.
//   LEAN_RING_3: three stages (the launches that put one or two workgroups on a CU and lose no co-resident one to the third stage:
//     ConvTune::ring3_tiles / ring3_wgs).  Two units in flight, the wait in front of the barrier leaves the younger one's copies
//     outstanding (a counted vmcnt), the barrier is a bare s_barrier, and the copies of unit u + 2 go out in runs between the MFMA groups
//     of unit u.
//   LEAN_RING_W: a third stage for the WINDOW alone (the k = 3 128-row tile without the folded second conv, whose three full stages
//     would cost the CU its third workgroup; ConvTune::ring3_window, ring3_window_tiles), 51.2 KB.  LDS holds three window planes (each
//     with its zero row) and behind them two slab sets; unit j of a tile (j = u - u_begin) uses window slot j % 3 and slab set j % 2.
//     During unit j the slabs of unit j + 1 and then the window of unit j + 2 are issued; at the top of unit j + 1 the wave waits with
//     vmcnt(this wave's copies of ONE window run) -- loads return in order, so the slabs have landed and only the younger window stays
//     outstanding: the copy a unit waits for shrinks from window + slabs to the slabs.
// Same MFMA order per accumulator, same epilogues: the three are bit-identical.
enum LeanRing { LEAN_RING_2 = 0, LEAN_RING_3 = 1, LEAN_RING_W = 2 };

// What a ring is on a shape: which shapes may take it, its bytes, the workgroups per CU its kernels are compiled for, and the slot of
// ldc_debug_lean_launches that counts its launches (0: none).  Read by the kernel and by the launcher.
template <typename SH, LeanRing RING>
struct LeanRingTraits {
  // three stages: the k = 3 and 1x1 kinds (one window run per plane).  Window ring: the tile it is built for, k = 3 on 128 x 64 without
  // the folded second conv.  (The 64 x 64 tile takes the full three-stage ring; with the fold it would fit the window ring -- 47.2 KB --
  // but measured 0.3 % slower per decode on it and was taken out again; with the fold on 128 x 64, and for 1x1 convs, three workgroups
  // of the window ring do not fit a CU: profiles/r10_ring_window.md.)
  static constexpr bool ok = RING == LEAN_RING_2 || (RING == LEAN_RING_3 && !SH::K4 && !SH::K7 && SH::NAW1 == 0) ||
                             (RING == LEAN_RING_W && SH::K3 && SH::TM == 2 && !SH::RF && SH::NAW1 == 0);
  static constexpr int STAGES = RING == LEAN_RING_2 ? 2 : 3;                       // window planes (per chunk of a unit)
  static constexpr int SLAB_SETS = RING == LEAN_RING_W ? 2 : STAGES;
  static constexpr int SLABS0 = STAGES * SH::B_OFF;                                // window ring: the planes back to back, slab set 0 behind them
  static constexpr int BYTES = RING == LEAN_RING_W ? SLABS0 + SLAB_SETS * SH::SLAB_BYTES : STAGES * SH::STAGE_BYTES;
  static constexpr int MIN_WGS = RING == LEAN_RING_3 ? 2 : 3;                      // __launch_bounds__
  static constexpr int COUNT_SLOT = RING == LEAN_RING_3 ? 5 : (RING == LEAN_RING_W ? 6 : 0);
};

// THE dynamic LDS of an instantiation.  The ring and the epilogue's staging share the front -- four waves' TM x 32 rows of 32 columns
// (fp32 where a residual is added: res32) + 16 bytes of padding per row --, whichever is larger; the folded LayerNorm's (mean, rstd)
// table of BM rows lies behind that, 16-aligned, at lean_ln_off.
constexpr bool lean_epi_res32(int epi) { return epi == LEAN_EPI_RES || epi == LEAN_EPI_GN_RES; }
template <typename T, int TM>
constexpr int lean_wave_staging(bool res32) { return TM * 32 * (32 * (res32 ? 4 : (int)sizeof(T)) + 16); }   // one wave's rows
template <typename T, typename SH, LeanRing RING>
constexpr int lean_front_bytes(bool res32) { return std::max(LeanRingTraits<SH, RING>::BYTES, 4 * lean_wave_staging<T, SH::TM>(res32)); }
template <typename T, typename SH, LeanRing RING>
constexpr int lean_ln_off(bool res32) { return (lean_front_bytes<T, SH, RING>(res32) + 15) / 16 * 16; }
template <typename T, typename SH, LeanRing RING>
constexpr size_t lean_lds_bytes(bool res32, bool ln = false) {
  return ln ? (size_t)lean_ln_off<T, SH, RING>(res32) + (size_t)SH::BM * 8 : (size_t)lean_front_bytes<T, SH, RING>(res32);
}
// (the layout in numbers: the window ring of the bf16 k = 3 128-row tile, two stages of it over its fp32 staging, the three stages of a
// 64-row 1x1 tile with the LayerNorm table behind them)
static_assert(lean_lds_bytes<__bf16, LeanShape<2, LEAN_K3, false>, LEAN_RING_W>(false) == 3 * 145 * 64 + 2 * 3 * 64 * 64, "window ring");
static_assert(lean_lds_bytes<__bf16, LeanShape<2, LEAN_K3, false>, LEAN_RING_2>(true) == 2 * (145 + 3 * 64) * 64, "ring over fp32 staging");
static_assert(lean_lds_bytes<float, LeanShape<1, LEAN_K1_LN, false>, LEAN_RING_3>(false, true) == 3 * (2 * 65 + 2 * 64) * 64 + 64 * 8, "LayerNorm table");

// a run of up to N copies of 1 KiB behind ONE M0 write: copy i lands at m0v + 1024 i and reads (base + voff_i + 1024 i); only the first
// `cnt` are issued (wave-uniform count: scalar branches, no exec masking).  The M0 write and its reader sit in one statement.
template <int N>
__device__ __forceinline__ void lean_dma_run(const char* base, unsigned m0v, unsigned cnt, unsigned v0, unsigned v1, unsigned v2) {
  if constexpr (N == 1) {
    // (a count of 0 / 1 is a boolean to the compiler, which then keeps it in a VGPR whatever readfirstlane says: branch in C++)
    if (cnt != 0u) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(v0), "s"(base), "s"(m0v) : "memory");
  } else if constexpr (N == 2) {
    asm volatile("s_mov_b32 m0, %3\n\ts_cmp_lt_u32 %4, 1\n\ts_cbranch_scc1 .Lq%=\n\tglobal_load_lds_dwordx4 %0, %2\n\t"
                 "s_cmp_lt_u32 %4, 2\n\ts_cbranch_scc1 .Lq%=\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n.Lq%=:"
                 ::"v"(v0), "v"(v1), "s"(base), "s"(m0v), "s"(cnt) : "memory", "scc");
  } else {
    asm volatile("s_mov_b32 m0, %4\n\ts_cmp_lt_u32 %5, 1\n\ts_cbranch_scc1 .Lq%=\n\tglobal_load_lds_dwordx4 %0, %3\n\t"
                 "s_cmp_lt_u32 %5, 2\n\ts_cbranch_scc1 .Lq%=\n\tglobal_load_lds_dwordx4 %1, %3 offset:1024\n\t"
                 "s_cmp_lt_u32 %5, 3\n\ts_cbranch_scc1 .Lq%=\n\tglobal_load_lds_dwordx4 %2, %3 offset:2048\n.Lq%=:"
                 ::"v"(v0), "v"(v1), "v"(v2), "s"(base), "s"(m0v), "s"(cnt) : "memory", "scc");
  }
}
// the same, all N copies (weight slabs)
template <int N>
__device__ __forceinline__ void lean_dma_all(const char* base, unsigned m0v, unsigned v0, unsigned v1, unsigned v2, unsigned v3) {
  if constexpr (N == 2) {
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024"
                 ::"v"(v0), "v"(v1), "s"(base), "s"(m0v) : "memory");
  } else if constexpr (N == 3) {
    asm volatile("s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %3\n\tglobal_load_lds_dwordx4 %1, %3 offset:1024\n\t"
                 "global_load_lds_dwordx4 %2, %3 offset:2048"
                 ::"v"(v0), "v"(v1), "v"(v2), "s"(base), "s"(m0v) : "memory");
  } else {
    asm volatile("s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %4\n\tglobal_load_lds_dwordx4 %1, %4 offset:1024\n\t"
                 "global_load_lds_dwordx4 %2, %4 offset:2048\n\tglobal_load_lds_dwordx4 %3, %4 offset:3072"
                 ::"v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(base), "s"(m0v) : "memory");
  }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// Epilogues of the lean kernel: the arithmetic of conv_device.h's (epilogue_rows / epilogue_rows_res / epilogue_gn_fused, TN = 1, two
// wave rows), re-ordered around what the device stamps of round 6 showed (profiles/r06_conv_issue.md): a fused GroupNorm epilogue took
// 14-22 k cycles against a 10 k-cycle K loop -- 2.8 k before the statistics were even published (the bias load's latency: every per-column
// constant is now fetched in the PROLOGUE, under the first copies), 4 k per poll round trip with two to four rounds (the polls of the up to
// three items of a tile went one after the other and the first one always came back before the peers' stores had landed: now one batch of
// loads per round for all items, behind a first nap of ConvTune::gn_nap0), and 4 k more with a residual (its loads were issued behind the
// exchange: now in front of it, they land during the wait).
// ---------------------------------------------------------------------------------------------------------------------------------
// sum over the 64 lanes, returned wave-uniform: four DPP adds (quad, quad pair, 8, 16 lanes: no LDS traffic) and the four row sums through
// v_readlane (the xor-shuffle tree of conv_device.h is six dependent ds_bpermute round trips per value)
__device__ __forceinline__ float lean_wave_sum(float v) {
  auto dpp = [](float x, auto ctrl) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, true)); };
  v += dpp(v, std::integral_constant<int, 0xB1>());    // quad_perm [1, 0, 3, 2]
  v += dpp(v, std::integral_constant<int, 0x4E>());    // quad_perm [2, 3, 0, 1]
  v += dpp(v, std::integral_constant<int, 0x141>());   // row_half_mirror
  v += dpp(v, std::integral_constant<int, 0x140>());   // row_mirror: every lane holds the sum of its row of 16
  const int iv = __float_as_int(v);
  return (__int_as_float(__builtin_amdgcn_readlane(iv, 0)) + __int_as_float(__builtin_amdgcn_readlane(iv, 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(iv, 32)) + __int_as_float(__builtin_amdgcn_readlane(iv, 48)));
}

// sum over aligned groups of G = 4 or 8 consecutive lanes, returned in every lane of the group (DPP only)
template <int G>
__device__ __forceinline__ float lean_group_sum(float v) {
  static_assert(G == 4 || G == 8, "quad or half row");
  auto dpp = [](float x, auto ctrl) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, true)); };
  v += dpp(v, std::integral_constant<int, 0xB1>());
  v += dpp(v, std::integral_constant<int, 0x4E>());
  if constexpr (G == 8) v += dpp(v, std::integral_constant<int, 0x141>());
  return v;
}

struct LeanCols {          // per-lane constants of this lane's output column (prefetched)
  float bias, gam, bet, sc, sh;
};

template <typename T, int TM, bool RES, typename KA>
__device__ __forceinline__ void lean_epilogue_plain(const KA& a, f32x16 (&acc)[TM][1], char* wave_lds, int m_wave0, int col_wave0, int M, float bv) {
  constexpr int TN = 1;
  typedef typename std::conditional<RES, float, T>::type TS;
  constexpr int PITCH = TN * 32 * (int)sizeof(TS) + 16;
  constexpr int EPL = 16 / (int)sizeof(T);          // output elements per lane in the row phase (16 bytes)
  constexpr int LPR = TN * 32 / EPL;                // lanes per row
  constexpr int RPS = 64 / LPR;                     // rows per sweep
  constexpr int NSW = TM * 32 / RPS;
  const int lane = (int)threadIdx.x & 63;
  const int rsub = lane / LPR, chunk = lane % LPR;
  const int col = col_wave0 + chunk * EPL;
  uint4 rres[RES ? NSW : 1];
  if constexpr (RES) {
#pragma unroll
    for (int sw = 0; sw < NSW; ++sw) {
      const int m = m_wave0 + sw * RPS + rsub;
      const bool ok = m < M && col < a.n;
      rres[sw] = *reinterpret_cast<const uint4*>(a.residual + ((size_t)(ok ? m : 0) * a.n + (ok ? col : 0)) * sizeof(T));
    }
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      store_out<TS>(wave_lds, (size_t)(row * PITCH) / sizeof(TS) + (lane & 31), acc[i][0][r] + bv);
    }
  // same wave wrote and reads: LDS executes a wave's operations in order
#pragma unroll
  for (int sw = 0; sw < NSW; ++sw) {
    const int row = sw * RPS + rsub;
    const int m = m_wave0 + row;
    uint4 v;
    if constexpr (!RES) {
      v = *reinterpret_cast<const uint4*>(wave_lds + row * PITCH + chunk * 16);
    } else {
      float f[EPL];
      const float* sp = reinterpret_cast<const float*>(wave_lds + (size_t)row * PITCH + chunk * EPL * 4);
#pragma unroll
      for (int e = 0; e < EPL; e += 4) {
        const float4 t = *reinterpret_cast<const float4*>(sp + e);
        f[e] = t.x; f[e + 1] = t.y; f[e + 2] = t.z; f[e + 3] = t.w;
      }
      const unsigned rw[4] = {rres[sw].x, rres[sw].y, rres[sw].z, rres[sw].w};
      if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) f[e] += __uint_as_float(rw[e]);
        v = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
      } else {
#pragma unroll
        for (int e = 0; e < EPL; e += 2) {
          f[e] += __uint_as_float(rw[e >> 1] << 16);
          f[e + 1] += __uint_as_float(rw[e >> 1] & 0xffff0000u);
        }
        v = make_uint4(hw_bf16x2(f[0], f[1]), hw_bf16x2(f[2], f[3]), hw_bf16x2(f[4], f[5]), hw_bf16x2(f[6], f[7]));
      }
    }
    if (m < M && col < a.n) *reinterpret_cast<uint4*>(a.y + ((size_t)m * a.y_ld + col) * sizeof(T)) = v;
  }
}

// Fused GroupNorm apply (conv_device.h: epilogue_gn_fused explains the exchange): same statistics, same summation order, same affine.
// NR = rounds of 64 granules an (item, group) may need (the launcher checks).
// `between` runs once the statistics are published and the residual is requested (the folded second conv's output goes out there: its
// LDS transpose and stores take ~2.4 k cycles of the ~6 k the exchange needs anyway).
template <typename T, int TM, bool RES, typename KA, typename F>
__device__ __forceinline__ void lean_epilogue_gn(const KA& a, f32x16 (&acc)[TM][1], char* wave_lds, int m_wave0, int col_wave0, int M, int m0, int BM,
                                                 int wm, const LeanCols& cl, GnStamp& gstamp, const bool stamp_on, F&& between) {
  constexpr int TN = 1, WM = 2, NR = 2;
  const int lane = (int)threadIdx.x & 63;
  const int b_first = (int)fdiv((unsigned)m0, a.lrows_div);
  const int b_last = (int)fdiv((unsigned)(min(m0 + BM, M) - 1), a.lrows_div);
  const int nit = b_last - b_first + 1;            // items of this tile (<= 3)
  const int m_split = (b_first + 1) * a.L_rows, m_split2 = m_split + a.L_rows;
  const int cpg = a.gn_cpg;                        // a multiple of 32
  const int sub_n = cpg >> 5, nc32 = a.n >> 5;
  const int mt = m0 / BM;
  const int c32 = col_wave0 >> 5;
  const float bv = cl.bias;
  // row-phase geometry (also the residual's)
  typedef typename std::conditional<RES, float, T>::type TS;
  constexpr int PITCH = TN * 32 * (int)sizeof(TS) + 16;
  constexpr int EPL = 16 / (int)sizeof(T);
  constexpr int LPR = TN * 32 / EPL;
  constexpr int RPS = 64 / LPR;
  constexpr int NSW = TM * 32 / RPS;
  const int rsub = lane / LPR, chunk = lane % LPR;
  const int col = col_wave0 + chunk * EPL;
  // 1. publish this wave's partial statistics, one granule pair per item of the tile
  for (int bb = b_first; bb <= b_last; ++bb) {
    const int lo = bb * a.L_rows, hi = min(lo + a.L_rows, M);
    float s = 0.f, ss = 0.f;
    if (nit == 1 && m0 + BM <= M) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = acc[i][0][r] + bv;
          s += v;
          ss = fmaf(v, v, ss);
        }
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m_wave0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (m >= lo && m < hi) {
            const float v = acc[i][0][r] + bv;
            s += v;
            ss = fmaf(v, v, ss);
          }
        }
    }
    s = lean_wave_sum(s);
    ss = lean_wave_sum(ss);
    if (lane == 0 && c32 < nc32) {
      const int mslot = mt - lo / BM;
      char* dst = a.gn_part + ((((size_t)bb * a.gn_mslots + mslot) * WM + wm) * nc32 + c32) * 16;
      store16_wt(dst, make_uint4(1u, __float_as_uint(s), 1u, __float_as_uint(ss)));
    }
  }
  if (stamp_on) gstamp.t_pub = __builtin_amdgcn_s_memtime();
  // the residual rows of the row phase: requested now, they land while the statistics are exchanged
  u32x4_t rres[RES ? NSW : 1];
  const bool has_res = RES && a.residual != nullptr;
  if constexpr (RES) {
#pragma unroll
    for (int sw = 0; sw < NSW; ++sw) {
      const int m = m_wave0 + sw * RPS + rsub;
      const bool ok = m < M && col < a.n;
      rres[sw] = u32x4_t{0u, 0u, 0u, 0u};
      if (has_res) {
        const uint4 t = *reinterpret_cast<const uint4*>(a.residual + ((size_t)(ok ? m : 0) * a.n + (ok ? col : 0)) * sizeof(T));
        rres[sw] = u32x4_t{t.x, t.y, t.z, t.w};
      }
    }
  }
  between();
  // 2. gather: one batch of L1-bypassing loads per round for every item of the tile that is still incomplete
  const int g = (col_wave0 < a.n ? col_wave0 : 0) / cpg;   // this wave's group (wave-uniform)
  const float inv_n = 1.0f / ((float)a.L_rows * (float)cpg);
  const char* src[3][NR];
  bool mine[3][NR];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int bb = min(b_first + k, b_last);
    const int lo = bb * a.L_rows, hi = min(lo + a.L_rows, M);
    const int total = ((hi - 1) / BM - lo / BM + 1) * WM * sub_n;   // granule pairs of (item bb, group g)
    const char* base = a.gn_part + (size_t)bb * a.gn_mslots * WM * nc32 * 16 + (size_t)g * sub_n * 16;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int l = r * 64 + lane;
      mine[k][r] = k < nit && l < total;
      const int ms_wm = mine[k][r] ? l / sub_n : 0, sub = mine[k][r] ? l - ms_wm * sub_n : 0;
      src[k][r] = base + ((size_t)ms_wm * nc32 + sub) * 16;
    }
  }
  u32x4_t gv[3][NR];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int r = 0; r < NR; ++r) gv[k][r] = u32x4_t{1u, 0u, 1u, 0u};
  bool have[3] = {false, nit < 2, nit < 3};
  bool poisoned = false;
  const unsigned long long t0 = wall_clock64();
  for (int z = 0; z < a.gn_nap0; ++z) __builtin_amdgcn_s_sleep(1);
  for (unsigned spins = 0;; ++spins) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (!have[k]) {
#pragma unroll
        for (int r = 0; r < NR; ++r)
          if (r == 0 || __builtin_amdgcn_readfirstlane((int)__any(mine[k][r]))) load16_sc1_issue(gv[k][r], src[k][r]);
      }
    wait_vm0();
    if (stamp_on) { if (!gstamp.polls) gstamp.t_first = __builtin_amdgcn_s_memtime(); ++gstamp.polls; }
    bool all = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (!have[k]) {
        bool ok = true;
#pragma unroll
        for (int r = 0; r < NR; ++r) ok = ok && (!mine[k][r] || (gv[k][r][0] == 1u && gv[k][r][2] == 1u));
        have[k] = __all(ok);
        all = all && have[k];
      }
    if (all) break;
    for (int z = 0; z < a.gn_nap; ++z) __builtin_amdgcn_s_sleep(1);
    const bool flagged = (spins & 255u) == 255u && a.fail_flag && __hip_atomic_load(a.fail_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
    if (flagged || wall_clock64() - t0 > 50000000ull) {   // 0.5 s (or an earlier launch of this call already gave up): raise the flag, poison the output
      if (lane == 0 && a.fail_flag && !flagged) __hip_atomic_store(a.fail_flag, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      poisoned = true;
      break;
    }
  }
  if (stamp_on) gstamp.t_done = __builtin_amdgcn_s_memtime();
  float ca[3] = {0.f, 0.f, 0.f}, cb[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k >= nit) continue;   // (wave-uniform)
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (mine[k][r]) {
        s += __uint_as_float(gv[k][r][1]);
        ss += __uint_as_float(gv[k][r][3]);
      }
    if (poisoned) s = __uint_as_float(0x7fc00000u);
    s = lean_wave_sum(s);
    ss = lean_wave_sum(ss);
    const float mean = s * inv_n;
    const float rstd = rsqrtf(fmaxf(ss * inv_n - mean * mean, 0.0f) + 1e-5f);
    float a1 = rstd * cl.gam, b1 = cl.bet - mean * a1;
    if (a.gn_ss) {
      a1 *= cl.sc;
      b1 = b1 * cl.sc + cl.sh;
    }
    ca[k] = a1; cb[k] = b1;
  }
  if (nit < 2) { ca[1] = ca[0]; cb[1] = cb[0]; }
  if (nit < 3) { ca[2] = ca[1]; cb[2] = cb[1]; }
  // 3. normalise, SiLU, stage
  if (nit == 1) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const float o = fast_silu(fmaf(acc[i][0][r] + bv, ca[0], cb[0]));
        store_out<TS>(wave_lds, (size_t)(row * PITCH) / sizeof(TS) + (lane & 31), o);
      }
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const bool second = m_wave0 + row >= m_split, third = m_wave0 + row >= m_split2;
        const float o = fast_silu(fmaf(acc[i][0][r] + bv, third ? ca[2] : (second ? ca[1] : ca[0]), third ? cb[2] : (second ? cb[1] : cb[0])));
        store_out<TS>(wave_lds, (size_t)(row * PITCH) / sizeof(TS) + (lane & 31), o);
      }
  }
  // 4. row phase (same wave wrote and reads: LDS executes a wave's operations in order)
  if constexpr (!RES) {
#pragma unroll
    for (int sw = 0; sw < NSW; ++sw) {
      const int row = sw * RPS + rsub;
      const int m = m_wave0 + row;
      const uint4 v = *reinterpret_cast<const uint4*>(wave_lds + row * PITCH + chunk * 16);
      if (m < M && col < a.n) *reinterpret_cast<uint4*>(a.y + ((size_t)m * a.y_ld + col) * sizeof(T)) = v;
    }
  } else {
    const bool out8 = (a.gn_out & 1) != 0;
#pragma unroll
    for (int sw = 0; sw < NSW; ++sw) {
      const int row = sw * RPS + rsub;
      const int m = m_wave0 + row;
      float f[EPL], rr[EPL];
      const float* sp = reinterpret_cast<const float*>(wave_lds + row * PITCH + chunk * EPL * 4);
#pragma unroll
      for (int e = 0; e < EPL; e += 4) {
        const float4 t = *reinterpret_cast<const float4*>(sp + e);
        f[e] = t.x; f[e + 1] = t.y; f[e + 2] = t.z; f[e + 3] = t.w;
      }
      if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) rr[e] = __uint_as_float(rres[sw][e]);
      } else {
#pragma unroll
        for (int e = 0; e < EPL; e += 2) {
          rr[e] = __uint_as_float(rres[sw][e >> 1] << 16);
          rr[e + 1] = __uint_as_float(rres[sw][e >> 1] & 0xffff0000u);
        }
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) f[e] += rr[e];
      if (a.rowstat_out) {   // per-row (sum, M2 about the block mean) of the values AS STORED, for a PreNorm folded into the consumer (epilogue_gn_fused)
        constexpr int G = 32 / EPL;
        float fr[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) fr[e] = (sizeof(T) == 2 && !(a.gn_out & 4)) ? bf16_to_f32(f32_to_bf16(f[e])) : f[e];
        float ps = 0.f, pq = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) ps += fr[e];
        ps = lean_group_sum<G>(ps);
        const float bm = ps * (1.0f / 32.0f);
#pragma unroll
        for (int e = 0; e < EPL; ++e) pq = fmaf(fr[e] - bm, fr[e] - bm, pq);
        pq = lean_group_sum<G>(pq);
        if ((chunk & (G - 1)) == 0 && m < M && col < a.n)
          *reinterpret_cast<float2*>(a.rowstat_out + ((size_t)m * (a.n >> 5) + (col >> 5)) * 2) = make_float2(ps, pq);
      }
      if (a.gn_out & 4) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) f[e] = fast_tanh(f[e]);
      }
      uint4 v;
      if constexpr (sizeof(T) == 4) {
        v = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
      } else {
        v = make_uint4(hw_bf16x2(f[0], f[1]), hw_bf16x2(f[2], f[3]), hw_bf16x2(f[4], f[5]), hw_bf16x2(f[6], f[7]));
      }
      if constexpr (sizeof(T) == 2) {
        if (out8) {   // OCP e4m3, saturating, from the un-rounded value (the consumer is an fp8 x fp8 conv)
          float c8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) c8[e] = fminf(fmaxf(f[e], -448.0f), 448.0f);
          int lo8 = 0, hi8 = 0;
          lo8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[0], c8[1], lo8, false);
          lo8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[2], c8[3], lo8, true);
          hi8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[4], c8[5], hi8, false);
          hi8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[6], c8[7], hi8, true);
          if (m < M && col < a.n) *reinterpret_cast<int2*>(a.y + (size_t)m * a.y_ld + col) = make_int2(lo8, hi8);
          continue;
        }
      }
      if (m < M && col < a.n) *reinterpret_cast<uint4*>(a.y + ((size_t)m * a.y_ld + col) * sizeof(T)) = v;
    }
  }
}


// LinearAttention context inside to_qkv (srcs/modules/unet.py:208-216: k = softmax_n(k), context[d][e] = sum_n k[d][n] v[e][n]).  The tile holds
// k_h (columns 0-31: the waves with wn = 0) and v_h (32-63: wn = 1) of ONE head for BM positions.  softmax over positions is shift-invariant
// while nothing clamps or underflows, so inside that range no maximum is needed: p = exp(min(k, kLinattnKClamp)), rounded to bf16 once; the same
// rounded values feed the column sums.  VALID RANGE (ldc_kernels.h: kLinattnKClamp, kLinattnKsumMin, kLinattnKsumMax): every column's sum of
// exp(k) in [2^-100, 1e26), which implies every k < 60.  Outside it the result would be silently wrong (entries above the clamp flattened to
// one weight; a column far below zero underflowing to 0 / 0).  Nothing is tested here: a clamped entry alone lifts its column's sum to e^60 >
// 1e26, so the tail that consumes the sums (attention.hip: linattn_tail_mfma_kernel) sees either fault in the sum it divides by and raises
// the context's failure word: the call fails with "device-side failure [ctx_range]" and fold_ctx 0 is the fallback.
// P^T and V^T go to LDS ([column][position], as attention.hip: linattn_ctx_mfma_kernel
// stages them), wave 0 multiplies them on the MFMA and adds the 32 x 32 partial context and the 32 partial sums to the item's workspace with
// fp32 atomics -- what the context launch did, without its launch, without the column-max pass in front of it and without k and v ever
// being written (two thirds of to_qkv's output).  A tile that straddles items makes one pass per item with the other items' positions zeroed.
template <int TM, typename KA>
__device__ __forceinline__ void lean_epilogue_qkv_ctx(const KA& a, f32x16 (&acc)[TM][1], char* lds, int m0, int M, int wm, int wn, int head) {
  constexpr int BM = TM * 64, P = BM + 8, D = 32, HD = 128;
  unsigned short* spT = reinterpret_cast<unsigned short*>(lds);             // [32][P]
  unsigned short* svT = spT + 32 * P;
  const int tid = (int)threadIdx.x, lane = tid & 63, i32 = lane & 31, g = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b_first = (int)fdiv((unsigned)m0, a.lrows_div);
  const int b_last = (int)fdiv((unsigned)(min(m0 + BM, M) - 1), a.lrows_div);
  for (int bb = b_first; bb <= b_last; ++bb) {
    const int lo = bb * a.L_rows, hi = min(lo + a.L_rows, M);
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
        const int m = m0 + rl;
        const bool in = m >= lo && m < hi;
        if (wn == 0) {
          const unsigned short pb = in ? hw_bf16(__expf(fminf(acc[i][0][r], kLinattnKClamp))) : (unsigned short)0;
          ps += __uint_as_float((unsigned)pb << 16);
          spT[i32 * P + rl] = pb;
        } else {
          svT[i32 * P + rl] = in ? hw_bf16(acc[i][0][r]) : (unsigned short)0;
        }
      }
    float* wsb = a.qkv_ctx_ws + (size_t)bb * a.qkv_ctx_stride;
    if (wn == 0) {
      ps += __shfl_xor(ps, 32);
      if (lane < 32) atomicAdd(&wsb[HD + head * D + i32], ps);
    }
    __syncthreads();
    if (wave == 0) {
      f32x16 c;
#pragma unroll
      for (int r = 0; r < 16; ++r) c[r] = 0.f;
#pragma unroll
      for (int sx = 0; sx < BM / 16; ++sx) {
        const uint4 pa = *reinterpret_cast<const uint4*>(&spT[i32 * P + 16 * sx + 8 * g]);
        const uint4 vb = *reinterpret_cast<const uint4*>(&svT[i32 * P + 16 * sx + 8 * g]);
        mfma_step<__bf16>(c, pa, vb);
      }
      float* ctx = wsb + 2 * HD + (size_t)head * D * D;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int d = (r & 3) + 8 * (r >> 2) + 4 * g;
        atomicAdd(&ctx[d * D + i32], c[r]);
      }
    }
    __syncthreads();   // the staging is free for the next item of the tile
  }
}

typedef const __attribute__((address_space(3))) u32x4_t* lds_u4_cptr;
__device__ __forceinline__ uint4 lean_lds16(unsigned addr) {   // ds_read_b128 from a raw LDS byte address (no symbol to add: the offset folds into the instruction)
  const u32x4_t v = *reinterpret_cast<lds_u4_cptr>(addr);
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// "the unit at the top of the ring has landed" with the younger copies left in flight: at most MUL x (this wave's window copies per
// run) + FIX copies outstanding -- an immediate, chosen by a scalar switch; loads return in order, so anything else outstanding only
// makes the wait stricter
template <int NAW, int MUL, int FIX>
__device__ __forceinline__ void lean_wait_keep(const unsigned wcnt) {
  if (NAW >= 3 && wcnt == 3u) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * MUL + FIX) : "memory");
  else if (NAW >= 2 && wcnt == 2u) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * MUL + FIX) : "memory");
  else if (wcnt == 1u) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MUL + FIX) : "memory");
  else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(FIX) : "memory");
}
// the barrier that hands a stage over: my fragment reads of the stage about to be overwritten are complete (lgkmcnt), nothing about
// the copy counter (a __syncthreads() fence would drain it again)
__device__ __forceinline__ void lean_handover() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");   // (nothing of the next phase moves in front of the barrier)
}

template <typename T, int TM, int KIND, bool RF, int EPI, bool SK, LeanRing RING = LEAN_RING_2>
__global__ __launch_bounds__(256, (LeanRingTraits<LeanShape<TM, KIND, RF>, RING>::MIN_WGS)) void conv_lean_kernel(const ConvKArgs a, const LeanGeom g) {
  using SH = LeanShape<TM, KIND, RF>;
  using RT = LeanRingTraits<SH, RING>;
  constexpr bool R3 = RING == LEAN_RING_3, RW = RING == LEAN_RING_W;
  static_assert(RT::ok, "this ring is not for this shape (LeanRingTraits)");
  static_assert(!RW || 3 * lean_lds_bytes<T, SH, RING>(lean_epi_res32(EPI)) <= 160 * 1024,
                "window ring: three workgroups of it (ring or epilogue staging, whichever is larger) fit a CU's 160 KB of LDS");
  constexpr int TN = 1, WM = 2, WN = 2, NW = 4, TG = SH::TG, KC = SH::KC, NS = SH::NS, NSB = SH::NSB, NAW = SH::NAW;
  constexpr int BM = SH::BM, BN = SH::BN, STAGE = SH::STAGE_BYTES, PLANE = SH::PLANE_BYTES;
  constexpr int BKE = kRowBytes / (int)sizeof(T);
  constexpr bool LN = KIND == LEAN_K1_LN;
  constexpr unsigned kBias = 3072u;   // the copies' immediates (0 / 1024 / 2048 / 3072) also move the global address: offsets are pre-biased, the base is lowered
  static_assert(!RF || SH::K3, "the folded 1x1 conv rides on a k = 3 unit");
  static_assert((!SH::K4 && !SH::K7) || (EPI <= LEAN_EPI_RES && (!SK || SH::K4)), "k = 4 / 7: plain and residual epilogues; k = 7 is never split");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void* lptr_t;
  const unsigned lds_base = (unsigned)(size_t)(lptr_t)smem;

  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const unsigned bid = blockIdx.x;
  unsigned long long t_start = 0, t_pro = 0, t_loop = 0, t_tab = 0, t_dma = 0;
  GnStamp gst = {0ull, 0ull, 0ull, 0u};
  if (g.stamps) t_start = __builtin_amdgcn_s_memtime();
  unsigned long long* const kst_slot = kst_begin(a, tid, bid);   // timed-mode stamps
  if (g.debug & 8) return;
  // (through the constant address space: a uniform, invariant address -- ONE s_load_dwordx8; as a plain global pointer it is a vector load + readfirstlane)
  typedef const __attribute__((address_space(4))) LeanTile* tile_cptr;
  const tile_cptr tp = (tile_cptr)(unsigned long long)g.tiles + bid;
  LeanTile tl;
  tl.m0 = tp->m0; tl.n0 = tp->n0; tl.sk_k = tp->sk_k; tl.sk_tile = tp->sk_tile; tl.R_lo = tp->R_lo; tl.nrows = tp->nrows; tl.u_begin = tp->u_begin; tl.u_end = tp->u_end;
  const int M = a.B * a.L_rows;
  const int m0 = tl.m0, n0 = tl.n0, R_lo = tl.R_lo, nrows = tl.nrows;

  // ---- per-lane copy sources (chunk-independent): window rows, weight rows ----
  const int r16 = lane >> 2;
  const unsigned gslot = (unsigned)(((lane & 3) ^ ((r16 >> 2) & 3)) << 4);   // LDS slot (lane & 3) of piece row r16 holds this global 16-byte slot
  const unsigned ldb1 = (unsigned)a.C1 * (unsigned)sizeof(T), ldb2 = (unsigned)a.C2 * (unsigned)sizeof(T);
  unsigned vw[NAW];
  auto window_offsets = [&](const unsigned ldb) {   // (again at the switch to the second input tensor: three registers less across the K loop than keeping both sets)
#pragma unroll
    for (int i = 0; i < NAW; ++i) {
      int r = (wave * NAW + i) * 16 + r16;
      if (r >= nrows) r = 0;
      vw[i] = (unsigned)(R_lo + r) * ldb + gslot + kBias - (unsigned)(i < SH::NAW0 ? i : i - SH::NAW0) * 1024u;   // (the immediate of its place in its run)
    }
  };
  const unsigned wcnt = (unsigned)__builtin_amdgcn_readfirstlane(max(0, min(NAW, (nrows - wave * NAW * 16 + 15) >> 4)));
  const unsigned slab_bytes = (unsigned)a.n_pad * kRowBytes;       // one tap of one chunk
  unsigned vb[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int q = 0; q < NSB; ++q) {
    // slab q of a unit: tap q of the chunk (k = 3 / 4 / 7; k = 3, q = 3: the folded 1x1 conv's slab) | chunk q of the unit (1x1 convs)
    const unsigned slab = SH::TAPS ? (unsigned)q * slab_bytes : (unsigned)q * (unsigned)a.wtaps * slab_bytes;
    vb[q] = slab + (unsigned)(n0 + wave * 16 + r16) * kRowBytes + gslot + kBias - (unsigned)q * 1024u;
  }
  const int csw = a.C1 / BKE;                                // first chunk that comes from x2
  const int pc0 = SH::K7 ? tl.u_begin >> 1 : tl.u_begin * KC;   // (k = 7: never split, u_begin = 0)
  int pc = pc0;                                              // producer cursor: next chunk to copy
  const char* xb;                                            // window source of chunk pc, lowered by the bias
  if (pc0 >= csw && a.C2 > 0) {
    xb = a.x2 + (size_t)(pc0 - csw) * kRowBytes - kBias;
    window_offsets(ldb2);
  } else {
    xb = a.x1 + (size_t)pc0 * kRowBytes - kBias;
    window_offsets(ldb1);
  }
  const unsigned chunk_w = (unsigned)a.wtaps * slab_bytes;   // weight bytes of one chunk
  const char* wb = a.w + (size_t)pc0 * chunk_w - kBias;
  const unsigned m0_win = lds_base + (unsigned)(wave * NAW * 1024);
  const unsigned m0_b = lds_base + (unsigned)(SH::B_OFF + wave * NSB * 1024);
  if (g.stamps) t_tab = __builtin_amdgcn_s_memtime();

  // ---- the producer: four primitives, composed by every loop below (LDS offsets are literals at every call site) ----
  const unsigned wcnt0 = SH::NAW1 ? min(wcnt, (unsigned)SH::NAW0) : wcnt, wcnt1 = wcnt - wcnt0;
  auto copy_window = [&](const int kc, const unsigned off) {   // this wave's run(s) of the window of chunk pc + kc into the plane at LDS offset off
    lean_dma_run<SH::NAW0>(xb + kc * kRowBytes, m0_win + off, wcnt0, vw[0], vw[NAW > 1 ? 1 : 0], vw[NAW > 2 ? 2 : 0]);
    if constexpr (SH::NAW1 > 0) lean_dma_run<SH::NAW1>(xb + kc * kRowBytes, m0_win + off + (unsigned)(SH::NAW0 * 1024), wcnt1, vw[NAW > 3 ? 3 : 0], vw[NAW > 4 ? 4 : 0], 0u);
  };
  auto copy_slabs = [&](const unsigned m0v, const unsigned v3) {   // this wave's pieces of the slabs at the weight cursor to the M0 value m0v
    lean_dma_all<NSB>(wb, m0v, vb[0], vb[1], vb[2], v3);
  };
  auto next_window = [&](const int n) {   // the window cursor, n chunks on
    pc += n;
    xb += n * kRowBytes;
    if (pc == csw) {   // the concatenated input's second tensor from here on
      xb = a.x2 - kBias;
      window_offsets(ldb2);
    }
  };
  auto next_weights = [&](const size_t bytes) { wb += bytes; };
  // a whole unit into stage st of the staged rings
  auto issue = [&](const int st) {
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) copy_window(kc, (unsigned)(st * STAGE + kc * PLANE));
    if constexpr (SH::K7) {
      // taps 0-3 of the chunk into stage 0, taps 4-6 into stage 1 with the chunk's window once more; the fourth slab of the second group
      // is tap 4 again (conv_fast_body: "pointed at a valid one"): it meets the zero row
      if (st == 0) {
        copy_slabs(m0_b, vb[3]);
        next_weights((size_t)4 * slab_bytes);
        return;
      }
      copy_slabs(m0_b + (unsigned)(st * STAGE), vb[3] - 3u * slab_bytes);
      next_weights((size_t)3 * slab_bytes);
    } else {
      copy_slabs(m0_b + (unsigned)(st * STAGE), vb[3]);
      next_weights((size_t)KC * chunk_w);
    }
    next_window(KC);
  };
  // window ring: the window runs one unit ahead of the slabs, so the switch to the second input tensor follows the window that is being
  // issued (pc counts windows), the weight pointer the slabs
  auto issue_window = [&](const int slot) { copy_window(0, (unsigned)(slot * PLANE)); next_window(1); };
  auto issue_slabs = [&](const unsigned m0v) { copy_slabs(m0v, vb[3]); next_weights((size_t)chunk_w); };
  const bool second_unit = tl.u_begin + 1 < tl.u_end && !(g.debug & 16);
  if constexpr (RW) {       // window(u0), slabs(u0), window(u0 + 1)
    issue_window(0);
    issue_slabs(m0_b + (unsigned)(RT::SLABS0 - SH::B_OFF));
    if (second_unit) issue_window(1);
  } else {
    issue(0);
    if constexpr (R3) {     // two units in flight from the start
      if (second_unit) issue(1);
    }
  }
  if (g.stamps) t_dma = __builtin_amdgcn_s_memtime();
  // per-column constants of the epilogue, requested now (used behind the K loop: a bias fetched there cost the epilogue 2 k cycles of load latency)
  // (not with the folded second conv: its 32 extra accumulators leave no room -- five more live registers across the K loop tipped hipcc
  // into parking accumulators and spilling; that variant fetches them behind the loop)
  LeanCols cl = {0.f, 0.f, 0.f, 1.f, 0.f};
  auto fetch_cols = [&]() {
    const int ecol = n0 + wn * 32 + (lane & 31);
    const bool ok = ecol < a.n;
    const int cc = ok ? ecol : 0;
    if (a.bias && ok) cl.bias = a.bias[ecol];
    if constexpr (EPI == LEAN_EPI_GN || EPI == LEAN_EPI_GN_RES) {
      cl.gam = a.gn_gamma[cc]; cl.bet = a.gn_beta[cc];
      if (a.gn_ss) { cl.sc = a.gn_ss[cc] + 1.0f; cl.sh = a.gn_ss[a.n + cc]; }
    }
  };
  if constexpr (!RF) fetch_cols();

  if constexpr (LN) ln_row_stats<T, BM, NW * 64>(a, reinterpret_cast<float*>(smem + g.ln_off), m0, M, tid);   // folded PreNorm LayerNorm (conv_device.h)

  // ---- everything below runs under the first copies' latency ----
  // zero rows (one behind every plane of every stage; the window ring's planes lie back to back): STAGES x KC x 16 dwords
  if (tid < RT::STAGES * KC * 16) {
    const int st = tid / (KC * 16), rem = tid - st * (KC * 16);
    reinterpret_cast<unsigned*>(smem + st * (RW ? SH::B_OFF : STAGE) + (rem >> 4) * PLANE + SH::ZERO_OFF)[rem & 15] = 0u;
  }
  // fragment addresses of this lane (stage 0, plane 0): A[i][tap][k-half], B[k-half]; stage / plane / slab offsets are immediates
  const int kh = lane >> 5;
  const int leff = a.L_in << a.ups;
  unsigned a_ad[TM][SH::NTAP][2];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + (wm * TM + i) * 32 + (lane & 31);
    int rb = -1, rl = 0;
    if (m < M) {
      rb = (int)fdiv((unsigned)m, a.lrows_div);
      rl = m - rb * a.L_rows;
    }
    // gather_row (conv_device.h) for zero padding, branch-free: position u of the (upsampled) input, a window row or the zero row
    const int u0 = rl * a.stride - a.pad_left;
    const int rowb = rb * a.L_in - R_lo;
#pragma unroll
    for (int t = 0; t < SH::NTAP; ++t) {
      const int u = u0 + t * a.dil;
      const bool ok = rb >= 0 && (unsigned)u < (unsigned)leff && (!SH::K7 || t < 7);
      const int row = rowb + (u >> a.ups);
      const int sw = (row >> 2) & 3;
      a_ad[i][t][0] = lds_base + (unsigned)(ok ? row * kRowBytes + ((kh ^ sw) << 4) : SH::ZERO_OFF);
      a_ad[i][t][1] = lds_base + (unsigned)(ok ? row * kRowBytes + (((2 + kh) ^ sw) << 4) : SH::ZERO_OFF);
    }
  }
  unsigned b_ad[2];
  {
    const int nl = wn * 32 + (lane & 31);                       // column of the tile
    const int rowb = ((nl >> 4) * NSB) * 16 + (nl & 15);        // its LDS row in slab 0: [16-column group][slab][16 rows]
    const int sw = ((nl & 15) >> 2) & 3;
    b_ad[0] = lds_base + (unsigned)(SH::B_OFF + rowb * kRowBytes + ((kh ^ sw) << 4));
    b_ad[1] = lds_base + (unsigned)(SH::B_OFF + rowb * kRowBytes + (((2 + kh) ^ sw) << 4));
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.0f;
  f32x16 acc2[RF ? TM : 1][1];   // folded 1x1 conv
  if constexpr (RF) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[i][0][r] = 0.0f;
  }

  // (Round 6, measured and not kept -- both bit-identical, numbers in profiles/r06_conv_issue.md: fragment reads one group ahead of their
  // MFMAs, held there with sched_barrier: 60 -> 127 VGPRs, SQ_WAIT_INST_LDS + 55 %, decode 0.2 % slower -- three waves per SIMD already
  // cover the ds_read latency; the GroupNorm + SiLU arithmetic of the epilogue on packed fp32 instructions: decode 0.3 % slower.)
  auto compute = [&](const int st) {   // the MFMA chain of one unit: straight-line code, every LDS offset an immediate
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      const int kc = q / TG, t = SH::K7 ? st * TG + q : q % TG;   // (k = 7: stage = tap group)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        uint4 af[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = lean_lds16(a_ad[i][t][ks] + (unsigned)(st * STAGE + kc * PLANE));
        const uint4 bf = lean_lds16(b_ad[ks] + (unsigned)(st * STAGE + q * 1024));
#pragma unroll
        for (int i = 0; i < TM; ++i) mfma_step<T>(acc[i][0], af[i], bf);
      }
    }
    if constexpr (RF) {   // centre-tap window rows x the unit's fourth slab
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        uint4 af[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = lean_lds16(a_ad[i][1][ks] + (unsigned)(st * STAGE));
        const uint4 bf = lean_lds16(b_ad[ks] + (unsigned)(st * STAGE + NS * 1024));
#pragma unroll
        for (int i = 0; i < TM; ++i) mfma_step<T>(acc2[i][0], af[i], bf);
      }
    }
  };

  if (g.stamps) t_pro = __builtin_amdgcn_s_memtime();
  const int u_end = (g.debug & 16) ? min(tl.u_end, tl.u_begin + 1) : tl.u_end;
  const bool copies = !(g.debug & 1);
  // Two units per trip (stages 0, 1) and ONE loop exit, an odd last unit behind the loop: with a second exit in the middle of the body
  // (`if (u + 1 >= u_end) break;`) hipcc gives the accumulators different registers on the two paths and copies all of them -- 32 to 64
  // v_mov plus s_nop per unit -- whenever registers get tight (the folded second conv's variant: 168 VGPRs and spills).
  int u = tl.u_begin;
  if constexpr (R3 || RW) {
    // ---- the three-unit rings: ONE loop, two policies (what lies where, what is copied behind which MFMA group, what a wait keeps) ----
    constexpr int NG = NS + (RF ? 1 : 0);   // MFMA groups of a unit (a tap or a chunk each; the folded second conv's last)
    // the MFMA chain of one unit, group by group: window fragments at LDS offset woff, slab fragments at bx + boff (q = NS: centre tap x
    // fourth slab).  The fragments of group q + 1 are requested in front of the MFMAs of group q (the copies are a compiler-level memory
    // barrier: what is to overlap them has to stand in front of them); behind the MFMAs of group q, where on(q), goes copy(q).
    auto step = [&](const unsigned woff, const unsigned (&bx)[2], const unsigned boff, auto&& on, auto&& copy) {
      auto frag = [&](const int q, uint4 (&af)[2][TM], uint4 (&bf)[2]) {
        const int kc = q < NS ? q / TG : 0, t = q < NS ? q % TG : 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
          for (int i = 0; i < TM; ++i) af[ks][i] = lean_lds16(a_ad[i][t][ks] + woff + (unsigned)(kc * PLANE));
          bf[ks] = lean_lds16(bx[ks] + boff + (unsigned)(q * 1024));
        }
      };
      uint4 af[2][2][TM], bf[2][2];
      frag(0, af[0], bf[0]);
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        if (q + 1 < NG) frag(q + 1, af[(q + 1) & 1], bf[(q + 1) & 1]);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            if constexpr (RF) {
              if (q == NS) { mfma_step<T>(acc2[i][0], af[q & 1][ks][i], bf[q & 1][ks]); continue; }
            }
            mfma_step<T>(acc[i][0], af[q & 1][ks][i], bf[q & 1][ks]);
          }
        if (on(q)) {
          __builtin_amdgcn_sched_barrier(0);
          copy(q);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    };
    // Window ring: the two slab sets.  A holds the units at positions 0 and 2 of a trip, B the one at position 1; a trip is three units
    // and the set alternates per unit, so the sets' fragment addresses and M0 values are two register sets swapped once per trip.
    constexpr unsigned kSlabs0 = (unsigned)(RT::SLABS0 - SH::B_OFF);   // slab set 0, relative to m0_b / b_ad
    unsigned bA[2] = {b_ad[0] + kSlabs0, b_ad[1] + kSlabs0}, bB[2] = {bA[0] + (unsigned)SH::SLAB_BYTES, bA[1] + (unsigned)SH::SLAB_BYTES};
    unsigned mA = m0_b + kSlabs0, mB = mA + (unsigned)SH::SLAB_BYTES;
    // The unit at position pos of a trip (a literal); n1 / n2: the next unit / the one after it exists and is to be copied.
    //   full ring: unit j in stage j % 3; behind group q goes run q of the unit after the next (one window run per plane, then the
    //     slabs; what is left of the runs behind the last group); the wait keeps one whole unit: KC wcnt + NSB copies.
    //   window ring: at the top of unit j the copies in flight are, oldest first, ... slabs(j), window(j + 1); behind group 0 go the
    //     slabs of the next unit (into the other set), behind group 1 the window of the unit after it (into slot pos + 2) -- slabs
    //     first, so that the wait may keep exactly the window: wcnt copies.
    auto unit = [&](const int pos, const bool n1, const bool n2) {
      if constexpr (R3) {
        step((unsigned)(pos * STAGE), b_ad, (unsigned)(pos * STAGE), [&](const int) { return n2; }, [&](const int q) {
          constexpr int NP = KC + 1;   // copy runs of a unit
          const int st = (pos + 2) % 3;
#pragma unroll
          for (int p = 0; p < NP; ++p)
            if (p == q || (q == NG - 1 && p > q)) {
              if (p < KC) {
                copy_window(p, (unsigned)(st * STAGE + p * PLANE));
              } else {
                copy_slabs(m0_b + (unsigned)(st * STAGE), vb[3]);
                next_weights((size_t)KC * chunk_w);
                next_window(KC);
              }
            }
        });
      } else {
        step((unsigned)(pos * PLANE), pos == 1 ? bB : bA, 0u, [&](const int q) { return (q == 0 && n1) || (q == 1 && n2); }, [&](const int q) {
          if (q == 0) issue_slabs(pos == 1 ? mA : mB);
          else issue_window((pos + 2) % 3);
        });
      }
    };
    auto wait_keep = [&]() { lean_wait_keep<NAW, R3 ? KC : 1, R3 ? NSB : 0>(wcnt); };
    // Three units per trip (stages and window slots are immediates) and ONE loop exit (see above); inside the loop every unit has a
    // younger one to leave in flight
    while (u + 3 < u_end) {
      wait_keep(); lean_handover();
      unit(0, copies, copies);
      wait_keep(); lean_handover();
      unit(1, copies, copies);
      wait_keep(); lean_handover();
      unit(2, copies, copies && u + 4 < u_end);
      u += 3;
      if constexpr (RW) { const unsigned t0 = bA[0], t1 = bA[1], tm = mA; bA[0] = bB[0]; bA[1] = bB[1]; mA = mB; bB[0] = t0; bB[1] = t1; mB = tm; }
    }
    // the last one to three units (workgroup-uniform: every wave meets the same barriers); the very last wait drains the counter
    const int left = u_end - u;
    if (left >= 1) {
      if (left >= 2) wait_keep(); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lean_handover();
      unit(0, copies && left >= 2, copies && left >= 3);
    }
    if (left >= 2) {
      if (left >= 3) wait_keep(); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lean_handover();
      unit(1, copies && left >= 3, false);
    }
    if (left >= 3) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lean_handover();
      unit(2, false, false);
    }
    u = u_end;
  }
  // ---- two stages: two units per trip, no fragment look-ahead, every unit drains the copy counter in front of a __syncthreads() ----
  while (u + 1 < u_end) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // my copies of unit u have landed
    __syncthreads();                                   // everybody's have; everybody is done with unit u - 1: its stage is free
    if (copies) issue(1);
    compute(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (u + 2 < u_end && copies) issue(0);
    compute(1);
    u += 2;
  }
  if (u < u_end) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    compute(0);
  }
  if (g.stamps) t_loop = __builtin_amdgcn_s_memtime();
  __syncthreads();   // every wave has consumed the last ring stage: LDS is free for the output transpose

  if constexpr (SK) {   // park the partial tile; the last slice to arrive sums all slices and carries on into the epilogue
    if (!splitk_park_and_sum<TM, TN, NW>(a, acc, smem, tl.sk_tile, tl.sk_k, wave, lane, tid)) return;
  }
  if constexpr (LN) ln_apply<TM, TN>(a, acc, reinterpret_cast<const float*>(smem + g.ln_off), wm * TM * 32, n0 + wn * 32, lane);
  {
    constexpr int wreg = lean_wave_staging<T, TM>(lean_epi_res32(EPI));
    char* wl = smem + (size_t)wave * wreg;
    const int mw = m0 + wm * TM * 32, cw = n0 + wn * 32;
    if (!(g.debug & 4)) {
      if constexpr (RF) fetch_cols();
      auto second_out = [&]() {
        if constexpr (RF) epilogue_rows_second<T, TM, TN>(a, acc2, wl, mw, cw, M);
      };
      if constexpr (EPI == LEAN_EPI_QKV) {
        // to_qkv with the LinearAttention context inside: tiles 0 / 1 are q (stored), every later tile is (k_h | v_h) of head (n0 - 128) / 64
        if (n0 < 128) lean_epilogue_plain<T, TM, false>(a, acc, wl, mw, cw, M, cl.bias);
        else if constexpr (sizeof(T) == 2) lean_epilogue_qkv_ctx<TM>(a, acc, smem, m0, M, wm, wn, (n0 - 128) >> 6);
      } else if constexpr (EPI == LEAN_EPI_GN) {
        lean_epilogue_gn<T, TM, false>(a, acc, wl, mw, cw, M, m0, BM, wm, cl, gst, g.stamps != nullptr, second_out);
      } else if constexpr (EPI == LEAN_EPI_GN_RES) {
        lean_epilogue_gn<T, TM, true>(a, acc, wl, mw, cw, M, m0, BM, wm, cl, gst, g.stamps != nullptr, second_out);
      } else {
        // (the launcher sends post-activations and the unfused GroupNorm statistics to conv_fast_kernel; the k column max rides on 1x1 convs only)
        if constexpr (!SH::TAPS) {
          if (a.colmax) epilogue_colmax<T, TM, TN>(a, acc, mw + 4 * (lane >> 5), cw + (lane & 31), m0, BM, M);
        }
        lean_epilogue_plain<T, TM, EPI == LEAN_EPI_RES>(a, acc, wl, mw, cw, M, cl.bias);
      }
    } else if (acc[0][0][0] == 12345.678f) {
      a.y[0] = 1;   // tuning aid: keep the accumulators live, store nothing
    }
  }
  kst_end(kst_slot, tid, bid, g.grid);
  if (g.stamps) {
    if (unsigned long long* o = stamp_phases(g.stamps, tid, bid, t_start, t_pro, t_loop, t_tab, t_dma)) {
      // fused GroupNorm apply (wave 0): ticks from the loop's end to statistics published / first poll back / all gathered (16 bits each, x 4), polls
      const auto d4 = [&](unsigned long long t) { return t > t_loop ? (unsigned long long)min((unsigned long long)0xffff, (t - t_loop) >> 2) : 0ull; };
      o[7] = d4(gst.t_pub) | (d4(gst.t_first) << 16) | (d4(gst.t_done) << 32) | ((unsigned long long)min(gst.polls, 0xffffu) << 48);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side: the tile table of a launch geometry (the dispatch order of conv_fast_body, evaluated once) and the launcher
// ---------------------------------------------------------------------------------------------------------------------------------
struct LeanKey {
  int v[27];
  bool operator<(const LeanKey& o) const { return memcmp(v, o.v, sizeof(v)) < 0; }
};

// conv_device.h: tile_window, on the host
static void lean_tile_window(const ConvKArgs& a, int m0, int BM, int M, int& R_lo, int& R_hi) {
  const int leff = a.L_in << a.ups;
  const int m_last = std::min(m0 + BM, M) - 1;
  int b = m0 / a.L_rows, l = m0 - b * a.L_rows;
  int u = l * a.stride - a.pad_left;
  u = std::max(0, std::min(u, leff - 1));
  R_lo = b * a.L_in + (u >> a.ups) - a.reflect_back;
  b = m_last / a.L_rows;
  l = m_last - b * a.L_rows;
  u = l * a.stride + (a.taps - 1) * a.dil - a.pad_left;
  u = std::max(0, std::min(u, leff - 1));
  R_hi = b * a.L_in + (u >> a.ups) + a.reflect_fwd;
  R_lo = std::max(R_lo, 0);
  R_hi = std::min(R_hi, a.B * a.L_in - 1);
}

// workgroup bid -> (m0, n0, split-K slice, tile slot): conv_fast_body's tile order (PH == 0), line by line, with plain divisions
static void lean_tile_of(int bid, const ConvKArgs& a, const FastGeom& gm, int BM, int BN, int& m0, int& n0, int& sk_k, int& sk_tile) {
  const int ntiles = gm.ntiles;
  sk_k = a.ksplit > 1 ? bid / ntiles : 0;
  sk_tile = bid - sk_k * ntiles;
  m0 = n0 = 0;
  if (gm.sk_xcd) {
    const int lg = a.ksplit == 4 ? 2 : 1;
    const int x = bid & 7, q = bid >> 3;
    sk_k = x & (a.ksplit - 1);
    const int per = gm.ntn >> (3 - lg);
    const int mt = q / std::max(1, per);
    const int nt = ((q - mt * per) << (3 - lg)) + (x >> lg);
    m0 = mt * BM;
    n0 = nt * BN;
    sk_tile = mt * gm.ntn + nt;
    return;
  }
  const int h = sk_tile;
  const int xcd = h & 7, slot = h >> 3;
  const int q = ntiles >> 3, r = ntiles & 7;
  const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  if (gm.item_major) {
    const int G = gm.ntn << 3;
    const int grp = h / G;
    const int hl = h - grp * G;
    int mt, nt;
    if (gm.item_major == 3 && grp < (gm.ntm >> 3)) {
      const int x = hl & 7, sl = hl >> 3;
      const int ml = sl / std::max(1, gm.ntn >> 2);
      mt = (grp << 3) + (ml << 1) + (x >> 2);
      nt = (x & 3) + ((sl - ml * (gm.ntn >> 2)) << 2);
    } else if (gm.item_major >= 2 && grp < (gm.ntm >> 3)) {
      const int sl = hl >> 3, per = gm.ntn >> 3;
      const int ml = sl / std::max(1, per);
      mt = (grp << 3) + ml;
      nt = (hl & 7) + ((sl - ml * per) << 3);
    } else if (grp < (gm.ntm >> 3)) {
      mt = (grp << 3) + (hl & 7);
      nt = hl >> 3;
    } else {
      const int rem = std::max(1, gm.ntm & 7);
      nt = hl / rem;
      mt = (grp << 3) + hl - nt * rem;
    }
    m0 = mt * BM;
    n0 = nt * BN;
  } else if (gm.m_fastest) {
    const int nt = t / gm.ntm;
    n0 = nt * BN;
    m0 = (t - nt * gm.ntm) * BM;
  } else {
    const int mt = t / gm.ntn;
    m0 = mt * BM;
    n0 = (t - mt * gm.ntn) * BN;
  }
}

// Round 6, second half: the dispatch order as a 2-D arrangement of the eight XCDs over (N stripe, M-tile residue), chosen per launch by
// the bytes the eight L2s would fetch: an XCD of an xm x xn arrangement (xm xn = 8) streams 1 / xn of the weights and 1 / xm of the
// windows, so the launch fetches  weights x xm + windows x xn.  conv_fast_body knows 8 x 1, 1 x 8 and (for whole groups of eight M tiles)
// 2 x 4; what is left of the M tiles after the last whole group fell back to an order in which every XCD touches most of the weights
// -- 19 of the 41 MB a 1024 -> 1024 launch at L = 75 fetched (19 M tiles of 64 rows: two groups and a remainder of three;
// profiles/r06_conv_pmc_classes.md).  With the table on the host the order is free: XCD (i, j) takes the tiles of N stripe j whose M tile
// is congruent to i mod xm, in (M, N) order -- all XCDs walk the items together, which is what the fused GroupNorm exchange wants (see
// conv_fast_body's comment on item-major dispatch; a dispatch band is xm <= 8 M tiles) -- and lists longer than an XCD's share of the
// workgroup ids (id mod 8, dealt round robin) hand their last tiles to the shorter ones.
// tile_of[bid] = mt * ntn + nt.  false: keep conv_fast_body's order (split-K, 8 x 1 arrangements, option conv_xcd_order = 0).
static bool lean_xcd_order(const ConvKArgs& a, const FastGeom& gm, size_t esz, std::vector<int>& tile_of, int* xn_out) {
  *xn_out = 0;
  const ConvTune* tn = a.tune;
  if (!tn || !tn->xcd_order || a.ksplit > 1 || gm.sk_xcd || gm.grid != gm.ntiles || gm.ntiles < 16) return false;
  const double w = (double)(a.C1 + a.C2) * a.wtaps * a.n_pad * (double)esz;
  const double act = (double)a.B * a.L_in * (a.C1 + a.C2) * (double)esz;
  int xn = 1;
  double best = 8.0 * w + act;
  for (int c = 2; c <= 8 && c <= gm.ntn; c *= 2) {
    const double cost = w * (8 / c) + act * c;
    if (cost < best) { best = cost; xn = c; }
  }
  if (tn->xcd_order > 1) xn = std::min(tn->xcd_order, 8);   // (tuning: 2 / 4 / 8 forced)
  if (xn == 1 || (xn & (xn - 1)) || xn > gm.ntn) return false;
  const int xm = 8 / xn, T = gm.ntiles;
  std::vector<std::vector<int>> want(8);
  for (int mt = 0; mt < gm.ntm; ++mt)
    for (int nt = 0; nt < gm.ntn; ++nt) want[(size_t)((mt % xm) * xn + (nt * xn) / gm.ntn)].push_back(mt * gm.ntn + nt);
  std::vector<int> spare;
  for (int k = 0; k < 8; ++k) {
    const size_t share = (size_t)((T - k + 7) / 8);
    while (want[(size_t)k].size() > share) { spare.push_back(want[(size_t)k].back()); want[(size_t)k].pop_back(); }
  }
  std::sort(spare.begin(), spare.end());
  size_t sp = 0;
  for (int k = 0; k < 8; ++k) {
    const size_t share = (size_t)((T - k + 7) / 8);
    while (want[(size_t)k].size() < share && sp < spare.size()) want[(size_t)k].push_back(spare[sp++]);
    if (want[(size_t)k].size() != share) return false;
    std::sort(want[(size_t)k].begin(), want[(size_t)k].end());
  }
  tile_of.assign((size_t)T, 0);
  for (int k = 0; k < 8; ++k)
    for (size_t sl = 0; sl < want[(size_t)k].size(); ++sl) tile_of[(size_t)k + 8 * sl] = want[(size_t)k][sl];
  *xn_out = xn;
  return true;
}

// the tile table of a launch geometry, on the host: entry b = what workgroup b does.  Returns the largest window of any tile.
// upc = units per chunk group (2 for k = 7: its two tap groups)
static int lean_build_tiles(const ConvKArgs& a, const FastGeom& gm, int BM, int BN, int KC, int M, int bke, int upc, std::vector<LeanTile>& h) {
  h.assign((size_t)gm.grid, LeanTile());
  const int nunits_all = ((a.C1 + a.C2) / bke) / KC * upc;
  int mx = 0;
  std::vector<int> tile_of;
  int xn = 0;
  const bool by_xcd = lean_xcd_order(a, gm, (size_t)(kRowBytes / bke), tile_of, &xn);
  if (getenv("LDC_VERBOSE") && atoi(getenv("LDC_VERBOSE")) >= 2)
    fprintf(stderr, "[ldc] lean tile table: %d x %d tiles of %d x %d, K %d x %d taps, L %d: %s (xn %d)\n", gm.ntm, gm.ntn, BM, BN, a.C1 + a.C2, a.wtaps, a.L_rows,
            by_xcd ? "XCD arrangement" : "conv_fast order", xn);
  for (int b = 0; b < gm.grid; ++b) {
    LeanTile& t = h[(size_t)b];
    if (by_xcd) {
      const int tt = tile_of[(size_t)b];
      t.m0 = (tt / gm.ntn) * BM; t.n0 = (tt % gm.ntn) * BN; t.sk_k = 0; t.sk_tile = tt;
    } else {
      lean_tile_of(b, a, gm, BM, BN, t.m0, t.n0, t.sk_k, t.sk_tile);
    }
    int lo = 0, hi = 0;
    lean_tile_window(a, t.m0, BM, M, lo, hi);
    t.R_lo = lo;
    t.nrows = hi - lo + 1;
    mx = std::max(mx, t.nrows);
    t.u_begin = a.ksplit > 1 ? (int)(((long long)nunits_all * t.sk_k) / a.ksplit) : 0;
    t.u_end = a.ksplit > 1 ? (int)(((long long)nunits_all * (t.sk_k + 1)) / a.ksplit) : nunits_all;
  }
  return mx;
}

// device copy of the tile table of this geometry (built on first use, kept for the life of the process: ~20 KB per geometry);
// *max_rows = the largest window of any tile.  nullptr on allocation failure.
static const LeanTile* lean_tile_table(const ConvKArgs& a, const FastGeom& gm, int BM, int BN, int KC, int M, int bke, int* max_rows, int upc = 1) {
  struct Entry { LeanTile* dev; int max_rows; };
  static std::map<LeanKey, Entry> cache;
  static std::mutex mu;
  LeanKey k;
  memset(&k, 0, sizeof(k));
  const int vals[24] = {gm.grid, gm.ntiles, gm.ntn, gm.ntm, a.ksplit, gm.sk_xcd, gm.item_major, gm.m_fastest, BM, BN, KC, M, a.B, a.L_rows, a.L_in,
                        a.stride, a.taps, a.dil, a.pad_left, a.ups, a.reflect_back, a.reflect_fwd, a.C1 + a.C2, bke};
  memcpy(k.v, vals, sizeof(vals));
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  k.v[23] = bke | (dev_id << 8);
  k.v[24] = a.wtaps * 65536 + a.n_pad;   // (with the order option: what lean_xcd_order decides on)
  k.v[25] = a.tune ? a.tune->xcd_order : 0;
  k.v[26] = upc;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(k);
  if (it != cache.end()) { *max_rows = it->second.max_rows; return it->second.dev; }
  std::vector<LeanTile> h;
  const int mx = lean_build_tiles(a, gm, BM, BN, KC, M, bke, upc, h);
  void* d = nullptr;
  if (hipMalloc(&d, h.size() * sizeof(LeanTile)) != hipSuccess) return nullptr;
  if (hipMemcpy(d, h.data(), h.size() * sizeof(LeanTile), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
  cache[k] = Entry{(LeanTile*)d, mx};
  *max_rows = mx;
  return (LeanTile*)d;
}

// one instantiation: its dynamic LDS (lean_lds_bytes) and the place of its LayerNorm table are its own
template <typename T, int TM, int KIND, bool RF, int EPI, bool SK, LeanRing RING>
static hipError_t launch_lean_kernel(const ConvKArgs& a, LeanGeom g, hipStream_t s) {
  using SH = LeanShape<TM, KIND, RF>;
  constexpr bool LN = KIND == LEAN_K1_LN;
  auto kern = conv_lean_kernel<T, TM, KIND, RF, EPI, SK, RING>;
  static bool lds_opt_in = false;
  if (!lds_opt_in) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    lds_opt_in = true;
  }
  g.ln_off = LN ? lean_ln_off<T, SH, RING>(lean_epi_res32(EPI)) : 0;
  constexpr size_t lds = lean_lds_bytes<T, SH, RING>(lean_epi_res32(EPI), LN);
  hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), lds, s, a, g);
  __atomic_fetch_add(&g_lean_launches[KIND], 1ll, __ATOMIC_RELAXED);
  // (slot 5: launches on the three-stage ring, of any kind; slot 6: launches on the window ring)
  if (LeanRingTraits<SH, RING>::COUNT_SLOT) __atomic_fetch_add(&g_lean_launches[LeanRingTraits<SH, RING>::COUNT_SLOT], 1ll, __ATOMIC_RELAXED);
  return hipGetLastError();
}
// ... on the ring the launcher chose, where the shape may take it (LeanRingTraits::ok; the launcher asks for no other)
template <typename T, int TM, int KIND, bool RF, int EPI, bool SK>
static hipError_t launch_lean_ring(LeanRing ring, const ConvKArgs& a, const LeanGeom& g, hipStream_t s) {
  using SH = LeanShape<TM, KIND, RF>;
  if constexpr (LeanRingTraits<SH, LEAN_RING_W>::ok) {
    if (ring == LEAN_RING_W) return launch_lean_kernel<T, TM, KIND, RF, EPI, SK, LEAN_RING_W>(a, g, s);
  }
  if constexpr (LeanRingTraits<SH, LEAN_RING_3>::ok) {
    if (ring == LEAN_RING_3) return launch_lean_kernel<T, TM, KIND, RF, EPI, SK, LEAN_RING_3>(a, g, s);
  }
  return launch_lean_kernel<T, TM, KIND, RF, EPI, SK, LEAN_RING_2>(a, g, s);
}

// workgroups of a kernel that fit one CU with this much dynamic LDS; 0 when the query fails
static int lean_ask_wgs(const void* fn, size_t lds) {
  int n = 0;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 256, lds) != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  return n;
}
// Workgroups of the k = 3 fused GroupNorm kernels of this tile and ring that fit one CU (occupancy query with their dynamic LDS; the
// worst of the epilogues), asked once.  0 when the query fails: no fused GroupNorm launch takes a deeper ring then.
template <typename T, int TM, bool RF, LeanRing RING>
static int lean_gn_wgs_per_cu() {
  static int cached = -1;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (cached >= 0) return cached;
  using SH = LeanShape<TM, LEAN_K3, RF>;
  int worst = 1 << 30;
  auto ask = [&](auto epi, auto sk) {
    constexpr int EPI = decltype(epi)::value;
    worst = std::min(worst, lean_ask_wgs(reinterpret_cast<const void*>(conv_lean_kernel<T, TM, LEAN_K3, RF, EPI, decltype(sk)::value, RING>),
                                         lean_lds_bytes<T, SH, RING>(lean_epi_res32(EPI))));
  };
  using GN = std::integral_constant<int, LEAN_EPI_GN>;
  using GN_RES = std::integral_constant<int, LEAN_EPI_GN_RES>;
  ask(GN(), std::false_type());
  if constexpr (!RF) {   // (the folded second conv: fused GroupNorm without residual, never split)
    ask(GN(), std::true_type());
    ask(GN_RES(), std::false_type());
    ask(GN_RES(), std::true_type());
  }
  cached = worst;
  return cached;
}
// A fused GroupNorm launch spins on its peers: unet_plan.cpp's residency rule (few_tiles) with the slots of the kernel it is to run on --
// the launch as a whole, or an item's tiles plus two dispatch groups, within the share of the chip a batch part can count on.
static bool lean_gn_resident(const ConvKArgs& a, const FastGeom& gm, int BM, int wgs_per_cu) {
  const long slots = (long)wgs_per_cu * a.tune->ring3_cu_share;
  const long item_tiles = (long)((a.L_rows + BM - 1) / BM + 1) * gm.ntn;
  return gm.grid <= slots || item_tiles + 16 * gm.ntn <= slots;
}

// The lean kernel for the launch launch_fast_cfg<T, 2, 2, TM, 1, TG, KC, 2, NA, RF> has decided (a, gm: its final arguments).
// *launched stays false where this launch is outside the lean kernel's shapes (the caller launches conv_fast_kernel).
template <typename T, int TM, int TG, int KC, bool RF>
static hipError_t launch_lean(const ConvKArgs& a, const FastGeom& gm, int M, hipStream_t s, bool* launched) {
#define LDC_LEAN_GO(KIND_, EPI_, SK_) return launch_lean_ring<T, TM, KIND_, RF, EPI_, SK_>(ring, a, g, s)
  *launched = false;
  if constexpr (kW8 || kFp8 || !((TG == 3 && KC == 1) || (TG == 1 && KC == 2) || (TG == 4 && KC == 1 && sizeof(T) == 2)) || (RF && TG != 3)) {
    return hipSuccess;
  } else if constexpr (TG == 4) {
    // round 7 (bf16): the stride-2 downsamples (k = 4, pad 1) and init_conv (k = 7, two tap groups per chunk), plain or residual epilogue
    const ConvTune* tn = a.tune;
    if (tn && (!tn->lean || !tn->lean_all)) return hipSuccess;
    const bool k4 = a.taps == 4 && a.stride == 2 && gm.ngroups == 1, k7 = a.taps == 7 && a.stride == 1 && gm.ngroups == 2;
    if (!(k4 || k7) || a.dil != 1 || a.ups || a.wtaps != a.taps) return hipSuccess;
    if (a.pad_mode != PAD_ZERO || a.post_act != ACT_NONE || a.gn_sum || a.gn_part || a.colmax || a.wscale || a.ln_s || a.qkv_ctx_ws || a.y2) return hipSuccess;
    constexpr int bke = kRowBytes / (int)sizeof(T);
    if ((a.C1 % bke) || (a.C2 % bke)) return hipSuccess;
    const bool sk = a.ksplit > 1, res = a.residual != nullptr;
    if (sk && (res || k7)) return hipSuccess;
    using SH4 = LeanShape<TM, LEAN_K4S2, false>;
    using SH7 = LeanShape<TM, LEAN_K7, false>;
    int max_rows = 0;
    const LeanTile* tiles = lean_tile_table(a, gm, SH4::BM, SH4::BN, 1, M, bke, &max_rows, k7 ? 2 : 1);
    if (!tiles) return hipErrorOutOfMemory;
    if (max_rows > (k4 ? SH4::PLANE_ROWS : SH7::PLANE_ROWS)) return hipSuccess;   // (odd input lengths: conv_fast_kernel)
    LeanGeom g;
    g.tiles = tiles; g.stamps = gm.stamps; g.debug = gm.debug; g.grid = gm.grid; g.ln_off = 0;
    const LeanRing ring = LEAN_RING_2;
    *launched = true;
    if (k4) {
      if (res) LDC_LEAN_GO(LEAN_K4S2, LEAN_EPI_RES, false);
      if (sk) LDC_LEAN_GO(LEAN_K4S2, LEAN_EPI_PLAIN, true);
      LDC_LEAN_GO(LEAN_K4S2, LEAN_EPI_PLAIN, false);
    }
    if (res) LDC_LEAN_GO(LEAN_K7, LEAN_EPI_RES, false);
    LDC_LEAN_GO(LEAN_K7, LEAN_EPI_PLAIN, false);
  } else {
    constexpr bool K3 = TG == 3;
    const ConvTune* tn = a.tune;
    if (tn && !tn->lean) return hipSuccess;
    if (gm.ngroups != 1 || a.pad_mode != PAD_ZERO || a.post_act != ACT_NONE || a.gn_sum || (K3 && a.colmax) || a.wscale) return hipSuccess;
    constexpr int bke = kRowBytes / (int)sizeof(T);
    if ((a.C1 % (bke * KC)) || (a.C2 % (bke * KC))) return hipSuccess;
    const bool gn = a.gn_part != nullptr;
    const bool res32 = a.residual != nullptr || (gn && (a.gn_out & 1));
    const int epi = gn ? (res32 ? LEAN_EPI_GN_RES : LEAN_EPI_GN) : (a.residual ? LEAN_EPI_RES : LEAN_EPI_PLAIN);
    const bool sk = a.ksplit > 1;
    const bool ln = a.ln_s != nullptr;
    if (ln && (K3 || sk || epi != LEAN_EPI_PLAIN)) return hipSuccess;
    const bool qctx = a.qkv_ctx_ws != nullptr;   // (bf16 to_qkv of four 32-wide heads with the LayerNorm folded in: the planner asks only then)
    if (qctx && (!ln || sizeof(T) != 2 || a.n != 384 || a.colmax)) return hipErrorInvalidValue;
    if (RF && (epi != LEAN_EPI_GN || sk)) return hipSuccess;
    if (gn && ((a.L_rows + (TM * 64) - 1) / (TM * 64) + 1) * 2 * (a.gn_cpg >> 5) > 128) return hipSuccess;   // (lean_epilogue_gn: two rounds of 64 granules per (item, group))
    if (sk && epi == LEAN_EPI_RES) return hipSuccess;
    if (!K3 && (epi == LEAN_EPI_GN || epi == LEAN_EPI_GN_RES)) return hipSuccess;
    using SH0 = LeanShape<TM, K3 ? LEAN_K3 : LEAN_K1, RF>;
    int max_rows = 0;
    const LeanTile* tiles = lean_tile_table(a, gm, SH0::BM, SH0::BN, KC, M, bke, &max_rows);
    if (!tiles) return hipErrorOutOfMemory;
    if (max_rows > SH0::PLANE_ROWS) return hipSuccess;   // (strided / dilated windows: conv_fast_kernel)
    LeanGeom g;
    g.tiles = tiles; g.stamps = gm.stamps; g.debug = gm.debug; g.grid = gm.grid; g.ln_off = 0;
    // The three-stage ring for the launches that put one or two workgroups on a CU (ConvTune::ring3_tiles; 0 = never), where
    // ConvTune::ring3_wgs workgroups of three stages still fit a CU's LDS: the third stage must not cost a co-resident workgroup.  With
    // two batch parts in flight the 128-row tiles (64.5 - 77 KB of ring: two per CU instead of three) lose more there than the loop
    // gains -- +1.1 % per decode -- while the 64-row tiles (52.5 KB: still three) gain 2.3 % (profiles/r09_ring3.md).
    // Where ring3_wgs workgroups of the full ring do NOT fit, the window ring where ring3_wgs workgroups of IT fit -- the k = 3
    // 128 x 64 tile (51.2 KB); ConvTune::ring3_window.  It costs no co-resident workgroup, so its grid threshold is its own
    // (ConvTune::ring3_window_tiles, 608: the 600-tile launches gain more from it than the 304-tile ones, profiles/r10_ring_window.md).
    // A fused GroupNorm launch takes either only if it stays resident with the occupancy of that ring's kernels (lean_gn_resident).
    const size_t cu_lds = (size_t)160 * 1024, wgs = (size_t)std::max(1, tn ? tn->ring3_wgs : 1);
    const bool fits3 = wgs * lean_lds_bytes<T, SH0, LEAN_RING_3>(res32, ln) <= cu_lds;
    LeanRing ring = LEAN_RING_2;
    if (tn && !(gm.debug & 1)) {
      if (tn->ring3_tiles > 0 && gm.grid <= tn->ring3_tiles && fits3 && (!gn || lean_gn_resident(a, gm, SH0::BM, lean_gn_wgs_per_cu<T, TM, RF, LEAN_RING_3>())))
        ring = LEAN_RING_3;
      if constexpr (LeanRingTraits<SH0, LEAN_RING_W>::ok) {
        if (ring == LEAN_RING_2 && tn->ring3_window && gm.grid <= tn->ring3_window_tiles && !fits3 && wgs * lean_lds_bytes<T, SH0, LEAN_RING_W>(res32) <= cu_lds &&
            (!gn || lean_gn_resident(a, gm, SH0::BM, lean_gn_wgs_per_cu<T, TM, false, LEAN_RING_W>())))
          ring = LEAN_RING_W;
      }
    }
    *launched = true;
    if constexpr (K3) {
      if constexpr (RF) {
        LDC_LEAN_GO(LEAN_K3, LEAN_EPI_GN, false);
      } else {
        if (epi == LEAN_EPI_PLAIN) { if (sk) LDC_LEAN_GO(LEAN_K3, LEAN_EPI_PLAIN, true); LDC_LEAN_GO(LEAN_K3, LEAN_EPI_PLAIN, false); }
        if (epi == LEAN_EPI_RES) LDC_LEAN_GO(LEAN_K3, LEAN_EPI_RES, false);
        if (epi == LEAN_EPI_GN) { if (sk) LDC_LEAN_GO(LEAN_K3, LEAN_EPI_GN, true); LDC_LEAN_GO(LEAN_K3, LEAN_EPI_GN, false); }
        if (sk) LDC_LEAN_GO(LEAN_K3, LEAN_EPI_GN_RES, true);
        LDC_LEAN_GO(LEAN_K3, LEAN_EPI_GN_RES, false);
      }
    } else {
      if constexpr (sizeof(T) == 2) {
        if (qctx) LDC_LEAN_GO(LEAN_K1_LN, LEAN_EPI_QKV, false);
      }
      if (ln) LDC_LEAN_GO(LEAN_K1_LN, LEAN_EPI_PLAIN, false);
      if (epi == LEAN_EPI_RES) LDC_LEAN_GO(LEAN_K1, LEAN_EPI_RES, false);
      if (sk) LDC_LEAN_GO(LEAN_K1, LEAN_EPI_PLAIN, true);
      LDC_LEAN_GO(LEAN_K1, LEAN_EPI_PLAIN, false);
    }
#undef LDC_LEAN_GO
  }
}
