// The chained pair of the bulk sites with every PEPS leg equal to 8 (forward X = R A, P = W X; backward Z1 = A Y, Tt = W Z1):
//
//   C1[(x, i2), (j1, y)] = sum_k   A1[(x, i2), k] B1[k, (j1, y)]          i2, j1 = 0..7;  x, y, k: per-walker live extents
//   C2[(i1, i2), (x, y)] = sum_{(k1, k2)} W[(i1, i2), (k1, k2)] C1[(x, k1), (k2, y)]     all four legs of W are 8
//
// tgemm_chain_kernel reaches these shapes through two 156-dword descriptors: reciprocal index splits per tile, a k walk with
// counters and multiplies, sixteen branched stores per tile.  Here the splits are shifts, stage 2 is eight unrolled rounds
// over K = 64, operand addresses are one per-lane base plus immediate or uniform offsets, and the argument block is a few
// dozen dwords.  Every element of C2 goes through the SAME sequence of v_mfma_f32_32x32x2f32 as in the generic kernel (rounds
// of eight k2 values, step q pairs 8 r + q with 8 r + 4 + q, then acc * alpha), so the two kernels store the same bytes;
// which lane, tile or wave holds an element is free, and is chosen so that no division is needed:
//   stage 1  a column tile is (j1 = 0..7) x (four values of y) -- ceil(y / 4) of them, the count of the generic 32-column tiles
//   stage 2  the columns (x, y) are split back through a table built once per block by enumerating (x, y) on a padded grid
// The intermediate lives in LDS as [64 rows (k1, k2)][pitch 97]: 96 columns are the capacity of the generic 6144-float buffer,
// the reads of stage 2 take immediate offsets, and a walker whose x * y exceeds 96 is walked in chunks of x exactly as there.
#pragma once
#include "tgemm.h"

namespace pepsgpu {

constexpr int TG_D8_COLS = TG_CHAIN_LDS_FLOATS / 64;   // 96
constexpr int TG_D8_PITCH = TG_D8_COLS + 1;

struct TgChainD8Args {
  const float *A1, *B1, *W;
  float *C2;
  int *flag;
  const int *xl, *kl, *yl, *sel;      // per-walker live extents of x, k, y (nullable: the static extent) and the W selector (nullable)
  const float *scale_in;              // nullable
  unsigned long long *flopc, *bytec;
  unsigned long long *stats;          // nullable (PEPSGPU_CHAIN_D8_STATS): {walkers computed, of them walked in chunks}
  long wA1, wB1, wW, wC2, sel_mul;
  int sel_inc, xmul, X, Ks, Ys;       // X, Ks, Ys: static extents of x, k, y
  int sA_i1, sA_i2;                   // stage 1, A operand: element strides of x and i2 (k is unit-stride, 16-byte loads)
  int sB_k, sB_j1, sB_j2;             // stage 1, B operand
  int sW_i1, sW_i2, sW_k1, sW_k2;     // W
  int sC_i1, sC_i2, sC_j1, sC_j2;     // C2: strides of i1, i2, x, y
  float alpha1, alpha2;
  int flop_stride;
};

__global__ __launch_bounds__(256, 6) void tgemm_chain_d8_kernel(const TgChainD8Args a) {
  __shared__ float s_mid[64 * TG_D8_PITCH];
  __shared__ int s_ocj[TG_D8_COLS];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // the per-walker words, written as the one batch of tg_entry_* (an unset slot reads tg_neutral_word, its value is dropped).
  // (The compiler still sinks the loads of y and x to their uses: three waits, not one; profiles/chain_d8_ab.md.)
  int x, K, y, wsel;
  float in_scale;
  {
    typedef const __attribute__((address_space(4))) int *cint_p;
    typedef const __attribute__((address_space(4))) float *cfloat_p;
    const int *const nz = &tg_neutral_word;
    const int *px = a.xl ? a.xl + b : nz, *pk = a.kl ? a.kl + b : nz, *py = a.yl ? a.yl + b : nz;
    const int *ps = a.sel ? a.sel + (long)b * a.sel_inc : nz;
    const float *pc = a.scale_in ? a.scale_in + b : reinterpret_cast<const float *>(nz);
    asm volatile("" ::"s"(px), "s"(pk), "s"(py), "s"(ps), "s"(pc));
    const int vx = *(cint_p)px, vk = *(cint_p)pk, vy = *(cint_p)py, vs = *(cint_p)ps;
    const float vc = *(cfloat_p)pc;
    asm volatile("" ::"s"(vx), "s"(vk), "s"(vy), "s"(vs), "s"(vc));
    x = a.xl ? max(0, min(a.X, vx * a.xmul)) : a.X;
    K = a.kl ? max(0, min(a.Ks, vk)) : a.Ks;
    y = a.yl ? max(0, min(a.Ys, vy)) : a.Ys;
    wsel = a.sel ? vs : 0;
    in_scale = a.scale_in ? vc : 1.f;
  }
  // the buffer test of tgemm_chain_kernel on these shapes: 64 x y floats, chunks of x when they do not fit
  int chunk = x;
  if (64 * x * y > TG_CHAIN_LDS_FLOATS) {
    if (y > TG_D8_COLS) {
      if (tid == 0) a.flag[b] = -1;
      return;
    }
    chunk = 1;
    while ((chunk + 1) * y <= TG_D8_COLS) ++chunk;     // = 96 / y (uniform; chunked walkers only)
  }
  if (tid == 0) a.flag[b] = 0;
  if (x <= 0 || y <= 0) return;
  if (a.flopc && tid == 0 && (b & (a.flop_stride - 1)) == 0) {     // (flop_stride: 1 or 64)
    const unsigned long long I1 = 8ull * x, J1 = 8ull * y, J2 = (unsigned long long)x * y;
    atomicAdd(a.flopc, 2ull * a.flop_stride * (I1 * J1 * K + 64ull * J2 * 64ull));
    if (a.bytec) atomicAdd(a.bytec, 4ull * a.flop_stride * (I1 * K + K * J1 + 64ull * 64ull + 64ull * J2));
  }
  if (a.stats && tid == 0) {
    atomicAdd(a.stats, 1ull);
    if (chunk < x) atomicAdd(a.stats + 1, 1ull);
  }
  const float *A1 = a.A1 + (long)b * a.wA1;
  const float *B1 = a.B1 + (long)b * a.wB1;
  const float *W = a.W + (long)b * a.wW + (long)wsel * a.sel_mul;
  float *C2 = a.C2 + (long)b * a.wC2;
  const float alpha1 = a.alpha1 * in_scale, alpha2 = a.alpha2;

  // column (xl, yv) of a chunk -> its offset in C2, for the stores of stage 2: enumerated on a grid padded to 32 or 128 values of y
  {
    const int sh = y <= 32 ? 5 : 7;
    const int yv = tid & ((1 << sh) - 1);
    for (int xl = tid >> sh; xl < chunk; xl += 256 >> sh)
      if (yv < y) s_ocj[xl * y + yv] = xl * a.sC_j1 + yv * a.sC_j2;
  }

  // what a lane addresses, fixed for the whole block
  const int rowA = (l31 >> 3) * a.sA_i1 + (l31 & 7) * a.sA_i2;        // stage 1: row (x = 4 ti + l31 / 8, i2 = l31 % 8) of a tile
  const int colB = (l31 >> 2) * a.sB_j1;                              // stage 1: column (j1 = l31 / 4, y = 4 tj + l31 % 4)
  const unsigned sBk = (unsigned)a.sB_k;
  const int ti2 = wave & 1;                                            // stage 2: a wave keeps its row tile of W
  unsigned wq[4];                                                      // byte offsets of W[(i1, i2), (0, 4 half + q)]
  {
    const int rowW = (ti2 * 4 + (l31 >> 3)) * a.sW_i1 + (l31 & 7) * a.sW_i2;
#pragma unroll
    for (int q = 0; q < 4; ++q) wq[q] = 4u * (unsigned)(rowW + (4 * half + q) * a.sW_k2);
  }
  const int rowC = ti2 * 4 * a.sC_i1 + 4 * half * a.sC_i2;            // stage 2: row (i1 = 4 ti2 + g, i2 = 4 half + e) of C2
  const int nr8 = (K + 7) >> 3;
  const int ntj1 = (y + 3) >> 2;

  for (int c0 = 0; c0 < x; c0 += chunk) {
    const int cn = min(chunk, x - c0);
    if (c0) __syncthreads();     // stage 2 of the chunk before has read the buffer
    // ---- stage 1: C1 of the rows c0 .. c0 + cn - 1 into LDS ----
    {
      const float *Ac = A1 + (long)c0 * a.sA_i1;
      const int nti = (cn + 3) >> 2;
      int ti = 0, tj = wave;
      while (tj >= ntj1) { tj -= ntj1; ++ti; }
      while (ti < nti) {
        const unsigned oab = (ti * 4 + (l31 >> 3) < cn) ? 4u * (unsigned)(rowA + ti * 4 * a.sA_i1) : 0u;
        const int yv = tj * 4 + (l31 & 3);
        const bool jv = yv < y;
        const unsigned obb = 4u * (unsigned)(colB + (jv ? yv : 0) * a.sB_j2);
        tg_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        auto load_round = [&](const int r, float (&av)[4], float (&bv)[4]) {
          const int kq = 8 * r + 4 * half;
          const float4 v = tg_ldf4(Ac, oab + 4u * (unsigned)min(kq, a.Ks - 4));
          av[0] = v.x; av[1] = v.y; av[2] = v.z; av[3] = v.w;
#pragma unroll
          for (int q = 0; q < 4; ++q) bv[q] = tg_ldf(B1, obb + 4u * __umul24((unsigned)min(kq + q, K - 1), sBk));
        };
        auto mfma_round = [&](const int r, float (&av)[4], float (&bv)[4]) {
          const int left = K - 8 * r;      // (uniform, >= 1) step q of the lower half-wave is k = 8 r + q, the upper half's is larger
          if (left < 8) {
            const int kq = 8 * r + 4 * half;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const bool ok = kq + q < K;
              av[q] = ok ? av[q] : 0.f;
              bv[q] = ok ? bv[q] : 0.f;
            }
          }
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], bv[0], acc, 0, 0, 0);
          if (left > 1) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], bv[1], acc, 0, 0, 0);
          if (left > 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], bv[2], acc, 0, 0, 0);
          if (left > 3) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], bv[3], acc, 0, 0, 0);
        };
        for (int r = 0; r < nr8; r += 2) {     // two rounds of loads in flight (all of them up to sixteen live k)
          float a0[4], b0[4], a1[4], b1[4];
          const bool two = r + 1 < nr8;
          load_round(r, a0, b0);
          if (two) load_round(r + 1, a1, b1);
          mfma_round(r, a0, b0);
          if (two) mfma_round(r + 1, a1, b1);
        }
        // accumulator 4 g + e = row (x = 4 ti + g, i2 = 4 half + e), column (j1 = l31 / 4, yv): element (8 i2 + j1, x y + yv) of the buffer
        if (jv) {
          float *o = s_mid + ((4 * half * 8 + (l31 >> 2)) * TG_D8_PITCH + ti * 4 * y + yv);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            if (ti * 4 + g < cn) {
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e * 8 * TG_D8_PITCH] = acc[4 * g + e] * alpha1;
            }
            o += y;
          }
        }
        tj += 4;
        while (tj >= ntj1) { tj -= ntj1; ++ti; }
      }
    }
    // ---- stage 2: the wave's 32 rows of W, fetched before the barrier ----
    float w[8][4];
    {
      // (the offsets are named as values of this iteration: hoisted out of the chunk loop, the 32 addresses became 64 registers)
      unsigned wo[4] = {wq[0], wq[1], wq[2], wq[3]};
      asm volatile("" : "+v"(wo[0]), "+v"(wo[1]), "+v"(wo[2]), "+v"(wo[3]));
#pragma unroll
      for (int k1 = 0; k1 < 8; ++k1) {
        const float *Wk = W + (long)k1 * a.sW_k1;
#pragma unroll
        for (int q = 0; q < 4; ++q) w[k1][q] = tg_ldf(Wk, wo[q]);
      }
    }
    __syncthreads();
    {
      const int Jt = cn * y;
      float *Cc = C2 + (long)c0 * a.sC_j1;
      for (int j0 = (wave >> 1) * 32; j0 < Jt; j0 += 64) {
        const int j = j0 + l31;
        const float *bp = s_mid + (4 * half * TG_D8_PITCH + j);
        tg_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int k1 = 0; k1 < 8; ++k1)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[k1][q], bp[(k1 * 8 + q) * TG_D8_PITCH], acc, 0, 0, 0);
        if (j < Jt) {     // sixteen stores under one mask: a uniform base per (g, e), one 32-bit byte offset per lane
          const unsigned oc = 4u * (unsigned)(s_ocj[j] + rowC);
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              *reinterpret_cast<float *>(reinterpret_cast<char *>(Cc + (long)(g * a.sC_i1 + e * a.sC_i2)) + oc) = acc[4 * g + e] * alpha2;
        }
      }
    }
  }
}

// The shape contract.  d1 / d2: the descriptors tgemm_chain_launch was given, before its own additions.
inline bool tgemm_chain_d8_accepts(const TGemmDesc &d1, const TGemmDesc &d2, const TGemmChainMap &mp, const float *A1, int allow_chunks,
                                   int dense, int f64acc) {
  if (!allow_chunks || dense || f64acc) return false;
  if (mp.mapK[0] != -1 || mp.mapK[1] != 2 || mp.mapK[2] != 4 || mp.mapJ[0] != -1 || mp.mapJ[1] != 1 || mp.mapJ[2] != 5) return false;
  if (d1.I[0] != 1 || d1.K[0] != 1 || d1.K[1] != 1 || d1.J[0] != 1 || d2.I[0] != 1 || d2.K[0] != 1 || d2.J[0] != 1) return false;
  if (d1.I[2] != 8 || d1.J[1] != 8 || d2.I[1] != 8 || d2.I[2] != 8 || d2.K[1] != 8 || d2.K[2] != 8) return false;
  if (d2.J[1] != d1.I[1] || d2.J[2] != d1.J[2] || d1.I[1] < 1 || d1.J[2] < 1 || d1.K[2] < 4) return false;
  if (!tg_vec_a(d1, A1)) return false;
  // live extents: x on I1[1] and J2[1], k on K1[2], y on J1[2] and J2[2], compacting (no mask), one word per entry; nothing else
  auto unset = [](const TgDyn &t) { return t.p == nullptr; };
  auto plain = [](const TgDyn &t) { return t.p == nullptr || (t.mask == 0 && t.div == 1); };
  auto same = [](const TgDyn &s, const TgDyn &t) { return s.p == t.p && (s.p == nullptr || (s.mul == t.mul && s.mask == t.mask && s.div == t.div)); };
  if (!unset(d1.dI[0]) || !unset(d1.dI[2]) || !unset(d1.dJ[0]) || !unset(d1.dJ[1]) || !unset(d1.dK[0]) || !unset(d1.dK[1])) return false;
  for (int s = 0; s < 3; ++s)
    if (!unset(d2.dI[s]) || !unset(d2.dK[s])) return false;
  if (!unset(d2.dJ[0]) || !plain(d1.dI[1]) || !plain(d1.dK[2]) || !plain(d1.dJ[2])) return false;
  if (!same(d1.dI[1], d2.dJ[1]) || !same(d1.dJ[2], d2.dJ[2])) return false;
  if ((d1.dK[2].p && d1.dK[2].mul != 1) || (d1.dJ[2].p && d1.dJ[2].mul != 1) || (d1.dI[1].p && d1.dI[1].mul < 1)) return false;
  if (d1.dynI || d2.dynI || d1.selA || d1.selB || d2.selB || d2.accumulate || d2.seldivA != 1) return false;
  // 24-bit strides (one multiply-add per operand address), non-negative; entries below 2^29 floats (32-bit byte offsets)
  const int st[] = {d1.sAi[1], d1.sAi[2], d1.sBk[2], d1.sBj[1], d1.sBj[2], d2.sAi[1], d2.sAi[2], d2.sAk[1], d2.sAk[2],
                    d2.sCi[1], d2.sCi[2], d2.sCj[1], d2.sCj[2]};
  for (int v : st)
    if (v < 0 || v >= (1 << 24)) return false;
  const long spanA = (long)d1.I[1] * d1.sAi[1] + 8l * d1.sAi[2] + d1.K[2];
  const long spanB = (long)d1.K[2] * d1.sBk[2] + 8l * d1.sBj[1] + (long)d1.J[2] * d1.sBj[2];
  const long spanW = 8l * (d2.sAi[1] + d2.sAi[2] + d2.sAk[1] + d2.sAk[2]);
  const long spanC = 8l * (d2.sCi[1] + d2.sCi[2]) + (long)d2.J[1] * d2.sCj[1] + (long)d2.J[2] * d2.sCj[2];
  return spanA < (1l << 29) && spanB < (1l << 29) && spanW < (1l << 29) && spanC < (1l << 29);
}

// d1 / d2 as tgemm_chain_launch has prepared them (flop counters set).  Returns what tgemm_chain_launch returns for the launch.
inline int tgemm_chain_d8_launch(hipStream_t s, const TGemmDesc &d1, const TGemmDesc &d2, const float *A1, const float *B1, const float *A2,
                                 float *C2, int *flag) {
  TgChainD8Args a;
  a.A1 = A1; a.B1 = B1; a.W = A2; a.C2 = C2; a.flag = flag;
  a.xl = d1.dI[1].p; a.kl = d1.dK[2].p; a.yl = d1.dJ[2].p; a.sel = d2.selA; a.scale_in = d1.scale_in;
  a.flopc = d1.flopc; a.bytec = d1.bytec;
  a.stats = tgemm_chain_d8_stats();
  a.wA1 = d1.wA; a.wB1 = d1.wB; a.wW = d2.wA; a.wC2 = d2.wC; a.sel_mul = d2.selA_mul;
  a.sel_inc = d2.selA_inc; a.xmul = d1.dI[1].mul; a.X = d1.I[1]; a.Ks = d1.K[2]; a.Ys = d1.J[2];
  a.sA_i1 = d1.sAi[1]; a.sA_i2 = d1.sAi[2];
  a.sB_k = d1.sBk[2]; a.sB_j1 = d1.sBj[1]; a.sB_j2 = d1.sBj[2];
  a.sW_i1 = d2.sAi[1]; a.sW_i2 = d2.sAi[2]; a.sW_k1 = d2.sAk[1]; a.sW_k2 = d2.sAk[2];
  a.sC_i1 = d2.sCi[1]; a.sC_i2 = d2.sCi[2]; a.sC_j1 = d2.sCj[1]; a.sC_j2 = d2.sCj[2];
  a.alpha1 = (float)d1.alpha; a.alpha2 = (float)d2.alpha;
  a.flop_stride = d1.flop_stride;
  hipLaunchKernelGGL(tgemm_chain_d8_kernel, dim3(d1.nbatch), dim3(256), 0, s, a);
  PG_CHECK_HIP(hipGetLastError());
  tg_chain_d8_count.fetch_add(1, std::memory_order_relaxed);
  // no entry is declined when a slice of the intermediate (64 y floats) fits the buffer at the static extent
  return d1.J[2] <= TG_D8_COLS ? 2 : 1;
}

}  // namespace pepsgpu
