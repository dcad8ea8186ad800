// conv_igemm_bf3s_kernel and its instantiations (the slow unit of the build: about five minutes).
//
// bf16x6 with PRE-SPLIT operands: activations and filters arrive as three bf16 planes each (swem_split_bf16x3_f32 /
// weight packing), so one input element is split once per tensor instead of once per (tap, N tile) use.  The k-loop
// then holds no vector arithmetic and no register staging at all: every 16-byte MFMA fragment row-run is moved
// HBM/L2 -> LDS by the buffer unit itself (buffer_load_dwordx4 ... lds: 64 lanes x 16 B = 64 consecutive rows of one
// [plane][k/8] image; padding taps use an out-of-range offset and land as zeros) while the waves read fragments and
// issue MFMAs.  The planes are CHANNEL-GROUP MAJOR, [plane][C/8][pixel][8 bf16] (filters [plane][K/8][Cout][8]), so the
// 64 lanes of one transfer read 64 consecutive 16-byte chunks = full cache lines (with NHWC planes each lane would
// touch its own line: measured 80-100 instead of 115-125 TFLOP/s for the register-staged kernel).
#include <type_traits>

#include "conv_mma16.h"

namespace {

// M16: the products run on v_mfma_f32_16x16x32_bf16 (one k-block = one MFMA k-step) instead of 32x32x16: the same cycles
// per FLOP, but the chip holds a higher clock on this shape under a dense bf16 load (MI355X_MICROARCH.md, DVFS item 7).
// NPL = 3: the six-product bf16x6 arithmetic on the hi/mid/lo planes; NPL = 1: plain bf16 (hi plane only, one product) --
// the mixed-precision mode of the training step (config.AMP), never the default.
// KG = k/8 groups per k-block: 4 (32 k, the default) or 2 (16 k: half the LDS per stage -- the 128x128 tile then fits three
// blocks of four waves per CU instead of one block; a k-block is half of a (channel block, tap) cell of the K order).
// Stream-K instantiations re-read the launch parameters in every segment from the kernel-argument segment through a pointer
// the optimiser cannot see through: left alone it hoists ~60 invariant scalar loads (descriptors, strides, epilogue
// pointers) out of the segment loop, keeps them all live across the k-loop and spills 70 of them -- 30 more vector registers
// and one resident block per CU instead of two.  (ConvP is the kernel's first argument: offset 0 of the segment.)
template <bool SK>
__device__ __forceinline__ const ConvP &segment_params(const ConvP &p) {
  if constexpr (SK) {
    typedef const __attribute__((address_space(4))) ConvP CP;
    CP *pp = (CP *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(pp));
    return *(const ConvP *)pp;
  } else {
    return p;
  }
}

// PF ("prefetched fragments", round 3): the wave keeps the MFMA fragments of k-block kb in registers and reads those of
// kb+1 from the LDS BETWEEN the MFMA groups of kb, into a second register set -- its matrix stream no longer stops for its
// own transfer requests, fragment reads and the stage hand-over, and a stage is free for the next transfer one iteration
// earlier (its fragments are in registers), so a ring of NST stages keeps NST-1 k-blocks in flight under the MFMAs instead of
// NST-2 + a hand-over in front of them.  16x16x32 MFMA, one or two planes.
template <int WM, int WN, int NST, int NW, bool M16, int NPL, int KG = 4, bool PF = false, bool SK = false, bool F16 = false>
// (second launch bound = resident blocks per CU the register allocation must allow: the 16-k-block tiles (KG == 2) exist to run
// THREE blocks of four waves per CU -- 168 registers; left at 2 the three-plane instantiation came out at 169 once the epilogue
// grew by the plane-residual path, and the exact-split leg lost 4 %)
__global__ __launch_bounds__(64 * NW, NW == 4 ? (KG == 2 ? 3 : 2) : 1) void conv_igemm_bf3s_kernel(ConvP p STAMP_ARG) {
  STAMP(0);
  static_assert(!F16 || NPL == 2, "fp16 planes come as a (hi, mid) pair");
  static_assert(KG == 4 || (KG == 2 && !M16 && NW == 4), "16-k blocks: four waves, 32x32x16 MFMA");
  static_assert(!PF || (M16 && NPL <= 2 && KG == 4), "prefetched fragments: 16x16x32 MFMA, at most two planes");
  // block tile 64WM x 64WN, NW waves as an (NW/2) x 2 grid, each owning TM x TN 32x32 accumulator tiles
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int TM = 4 * WM / NW, TN = WN;
  static_assert(TM >= 1 && TM * (NW / 2) * 32 == BM, "wave grid must tile the block");
  // slot stride per k/8 group: the 16x16x32 fragment read mixes two k/8 groups inside one 16-lane bank group, which is
  // conflict free when the stride is a multiple of 16 slots; the 32x32x16 read does not care (kept as it was)
  constexpr int SA = BM + (M16 ? 0 : 1), SB = BN + (M16 ? 0 : 1);
  constexpr int PA = KG * SA, PB = KG * SB;
  constexpr int NA = NPL * KG * WM, NB = NPL * KG * WN;  // 64-row fragment runs per k-block
  // NST LDS stages: the transfers run NST-1 k-blocks ahead of the MFMAs
  constexpr int NDMA = (NA + NB) / NW;             // transfers per wave per k-block
  static_assert(NW == KG || WM == WN, "split roles: half the waves move the A image, half the B image, the same count each");
  static_assert((NA + NB) % NW == 0, "every wave must issue the same number of transfers (counted vmcnt)");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4 *As = reinterpret_cast<uint4 *>(smem);  // [NST][3][PA]
  uint4 *Bs = As + NST * NPL * PA;              // [NST][NPL][PB]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  // ---- Stream-K.  A grid of T tiles on S resident-block slots runs ceil(T / S) rounds however few tiles the last one holds
  // (2x120x216x256 -> 256: 810 tiles of 128x128 on 512 slots = 1.58 -> 2 rounds; most other layers: ~410 blocks = one round
  // with a fifth of the slots empty).  Here the launch is sk_workers PERSISTENT blocks (every slot one), and worker v takes the
  // v-th equal share of the (tile, k-block) iterations, tiles in the XCD-aware order: the tail of a tile another worker began
  // (-> its partial sums go to the workspace), whole tiles, and the head of a last tile (-> this worker adds the partial
  // sums of the workers that follow, in their order: deterministic, and runs the epilogue).  The producer of a partial tile
  // works on it FIRST and never waits for anyone; the owner needs it LAST -- no worker waits on a worker that could be
  // waiting, and a worker that is not yet resident (other streams' kernels hold slots) is dispatched as earlier ones finish.
  // Hand-over across CUs / XCDs (per-XCD L2s are not coherent): the partial sums are stored and loaded past the caches
  // (sc0 sc1), the producer drains its stores (vmcnt(0) + block barrier) before its flag, flags are agent-scope atomics.
  constexpr bool sk = SK;   // (its own instantiation: the segment loop costs the plain kernel ~30 registers)
  long long sk_it = 0, sk_end = 0, sk_total = 0;
  int sk_v = 0;
  if (sk) {
    const int W_ = p.sk_workers, q8 = W_ >> 3, r8 = W_ & 7, xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
    sk_v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + local;   // an XCD's workers share a tile range
    sk_total = (long long)p.sk_mtiles * p.sk_ntiles * p.nkb;
    sk_it = sk_total * sk_v / W_;
    sk_end = sk_total * (sk_v + 1) / W_;
  }
  const ConvP &p_arg = p;
  for (;;) {   // segments of this worker (without stream-K: the one tile of this block)
  const ConvP &p = segment_params<SK>(p_arg);
  int tm, tn, seg_k0 = 0, seg_k1 = p.nkb, sk_tile = 0;
  if (sk) {
    if (sk_it >= sk_end) break;
    sk_tile = (int)(sk_it / p.nkb);
    seg_k0 = (int)(sk_it - (long long)sk_tile * p.nkb);
    seg_k1 = (int)min((long long)p.nkb, seg_k0 + (sk_end - sk_it));
    sk_it += seg_k1 - seg_k0;
    const int ng = p.sk_ntiles / p.xpn, G = p.sk_mtiles * ng;   // tile order of tile_coords
    const int jn = sk_tile / G, rem = sk_tile - jn * G;
    tm = rem / ng;
    tn = jn * ng + rem - tm * ng;
    __syncthreads();   // every wave has left the previous segment (its epilogue stages planes in the operand LDS)
  } else {
    tile_coords(tm, tn, p.xpn);
    tm += p.mt0;
  }
  const int m0 = tm * BM, n0 = tn * BN;

  auto src_rsrc = [&](int sidx) __attribute__((always_inline)) {
    const unsigned short *base = sidx == 0 ? p.xs[0] : (sidx == 1 ? p.xs[1] : p.xs[2]);
    const long long ps = sidx == 0 ? p.ps[0] : (sidx == 1 ? p.ps[1] : p.ps[2]);
    return raw_rsrc(base, (unsigned)(3 * ps * 2));
  };
  // (per-batch filter planes -- matching's value readout, a batched GEMM: tiles never straddle two batch items)
  const i32x4 rsw = raw_rsrc(p.wsplit + (p.w_bs ? (long long)(m0 / (p.Ho * p.Wo)) * p.w_bs : 0ll),
                             (unsigned)((long long)3 * p.Ncols * p.K * 2));
  const unsigned wplane = (unsigned)((long long)p.Ncols * p.K * 2);
  const unsigned wgroup = (unsigned)p.Ncols * 16u;  // bytes per k/8 group of the filter planes

  // rows served by this lane: run j covers rows j*64 + lane of the A (pixels) and B (filters) tiles
  int iy0[WM], ix0[WM], bidx[WM];
  const int HoWo = p.Ho * p.Wo;
#pragma unroll
  for (int j = 0; j < WM; ++j) {
    int m = m0 + j * 64 + lane;
    int b = fast_div(m, p.fd_howo_mul, p.fd_howo_sh);
    int rem = m - b * HoWo;
    int oy = fast_div(rem, p.fd_wo_mul, p.fd_wo_sh), ox = rem - oy * p.Wo;
    iy0[j] = tap_origin(p, oy);
    ix0[j] = tap_origin(p, ox);
    bidx[j] = m < p.M ? b : -1;
  }
  unsigned bvoff[WN];
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    int n = n0 + j * 64 + lane;
    bvoff[j] = n < p.Ncols ? (unsigned)n * 16u : OOB;
  }
#ifdef SWEM_PROLOGUE_STAMPS
  STAMP(6);
#endif
  // Each wave moves ONE k/8 group (g = wave & 3) of every plane: the slot -> (operand, plane, row run) map is then a
  // compile-time constant and the wave only adds its group's offsets, kept in scalars that advance by one add per k-block.
  // (With eight waves, waves 0-3 move the A image and 4-7 the B image.)  Scalar instructions share the wave's issue
  // slot with the MFMAs: the first version of this loop spent 24 % of its wave cycles on ~190 of them per k-block.
  const int g = wave % KG, half = wave / KG;   // (NW == KG: every wave moves both images of its group)
  unsigned avoff[WM];
  unsigned aplane = 0, agroup = 0;  // byte strides between the planes / the 8-channel groups of the current source
  unsigned a_base = 0;              // scalar offset of (current k-block, group g) in plane 0 of the current source
  unsigned w_base = 0;              // ... of the filter planes
  i32x4 rsa;
  // K order of this kernel: k = (ci / 32, ky, kx, ci % 32) over the concatenated input channels ("channel-block major";
  // the filter planes are packed in that order).  With the usual tap-major order (ky, kx, ci) a tap is one pass over all
  // input channels, so a block re-reads its pixels' neighbourhood KH*KW times, each time long after the last: with ~13
  // blocks per XCD the footprint of a pass exceeds the 4 MiB L2 and the activations are fetched once per tap (measured
  // on 2x30x54x1280 -> 512: 8 x filters + 9 x activations).  Here the KH*KW taps of one 32-channel block are
  // consecutive k-blocks and the re-reads hit the L2 right away.  The tap changes every k-block, so its per-lane cost
  // must be a couple of vector instructions: the lane keeps the pixel index of tap (0, 0) and a validity bit per tap;
  // the tap's offset is that index plus a wave-uniform delta (forward: +(ky W + kx); data gradient: -((ky >> s) W +
  // (kx >> s)) with s = stride - 1, because a valid tap has i = (o0 - k) / stride = (o0 >> s) - (k >> s)).
  const int dsh = (p.flags & SWEM_CONV_DGRAD) ? p.stride - 1 : 0;
  int pix0[WM];
  unsigned long long tmask[WM];
  // (round 5) the forward convolution's valid taps along an axis are the contiguous range  k in [max(0, -o0), min(K, lim - o0))
  // -- two bit ranges per row instead of KH + KW coordinate tests with their data-gradient branches (stamps: 2.8k of the 128x128
  // tile's 8.0k prologue cycles, 0.65k of the 64x64 tile's 4.0k); the generic loops serve the data gradient
  const bool fwd_taps = !(p.flags & SWEM_CONV_DGRAD) && p.KW < 32 && p.KH < 32;
#pragma unroll
  for (int j = 0; j < WM; ++j) {
    // bit (ky * KW + kx) = tap row ky valid AND tap column kx valid: KH + KW coordinate tests, not KH * KW
    unsigned long long mk = 0;
    if (fwd_taps) {
      auto range_bits = [](int o0, int K, int lim) __attribute__((always_inline)) {
        const int lo = o0 < 0 ? -o0 : 0, hi = lim - o0 < K ? lim - o0 : K;
        return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
      };
      const unsigned colv = range_bits(ix0[j], p.KW, p.W), rowv = range_bits(iy0[j], p.KH, p.H);
      for (int ky = 0; ky < p.KH; ++ky) mk |= ((rowv >> ky) & 1u) ? (unsigned long long)colv << (ky * p.KW) : 0ull;
    } else {
      unsigned colv = 0;
      for (int kx = 0; kx < p.KW; ++kx) {
        int ix;
        colv |= (tap_coord(p, ix0[j], kx, p.W, ix) ? 1u : 0u) << kx;
      }
      for (int ky = 0; ky < p.KH; ++ky) {
        int iy;
        if (tap_coord(p, iy0[j], ky, p.H, iy)) mk |= (unsigned long long)colv << (ky * p.KW);
      }
    }
    tmask[j] = bidx[j] >= 0 ? mk : 0ull;
  }
#ifdef SWEM_PROLOGUE_STAMPS
  STAMP(7);
#endif
  auto set_src = [&](const KPos &q) __attribute__((always_inline)) {
    const long long ps = q.src == 0 ? p.ps[0] : (q.src == 1 ? p.ps[1] : p.ps[2]);
    const int npx = q.src == 0 ? p.npx[0] : (q.src == 1 ? p.npx[1] : p.npx[2]);
    const int bsp = q.src == 0 ? p.bsp[0] : (q.src == 1 ? p.bsp[1] : p.bsp[2]);
    aplane = (unsigned)(ps * 2);
    agroup = (unsigned)npx * 16u;       // pixels in the plane * 16 bytes
    a_base = (unsigned)(q.ci0 / 8 + g) * agroup;
    rsa = src_rsrc(q.src);
#pragma unroll
    for (int j = 0; j < WM; ++j)
      pix0[j] = (bidx[j] < 0 ? 0 : bidx[j]) * bsp + (iy0[j] >> dsh) * p.W + (ix0[j] >> dsh);
  };
  auto set_tap = [&](const KPos &q) __attribute__((always_inline)) {
    const int t = q.ky * p.KW + q.kx;
    const int d = (q.ky >> dsh) * p.W + (q.kx >> dsh);
    const int delta = (p.flags & SWEM_CONV_DGRAD) ? -d : d;
#pragma unroll
    for (int j = 0; j < WM; ++j) avoff[j] = ((tmask[j] >> t) & 1ull) ? (unsigned)(pix0[j] + delta) * 16u : OOB;
  };
  int khalf = 0;   // KG == 2: which 16-channel half of the current (channel block, tap) cell
  auto advance = [&](KPos &q) __attribute__((always_inline)) {
    w_base += KG * wgroup;
    if (KG == 2) {
      khalf ^= 1;
      if (khalf) {                 // second half of the same cell: the same tap, the next two channel groups
        a_base += 2 * agroup;
        return;
      }
      a_base -= 2 * agroup;
    }
    if (++q.kx == p.KW) {
      q.kx = 0;
      if (++q.ky == p.KH) {
        q.ky = 0;
        q.ci0 += BK;
        a_base += 4 * agroup;
        const int cs = q.src == 0 ? p.c[0] : (q.src == 1 ? p.c[1] : p.c[2]);
        if (q.ci0 >= cs) {
          q.ci0 = 0;
          ++q.src;
          set_src(q);
        }
      }
    }
    set_tap(q);
  };
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
  const unsigned lds_a = lds0 + (unsigned)g * (SA * 16), lds_b = lds0 + NST * NPL * PA * 16 + (unsigned)g * (SB * 16);
  auto issue = [&](int stage) __attribute__((always_inline)) {
    const unsigned sa = lds_a + (unsigned)stage * (NPL * PA * 16), sb = lds_b + (unsigned)stage * (NPL * PB * 16);
    if (NW == KG || half == 0) {
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
        for (int j = 0; j < WM; ++j) dma16(rsa, sa + (pl * PA + j * 64) * 16, avoff[j], a_base + pl * aplane);
    }
    if (NW == KG || half == 1) {
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
        for (int j = 0; j < WN; ++j) dma16(rsw, sb + (pl * PB + j * 64) * 16, bvoff[j], w_base + pl * wplane);
    }
  };

  f32x16 acc[M16 ? 1 : TM][M16 ? 1 : TN];
  f32x4v acc16[M16 ? 2 * TM : 1][M16 ? 2 * TN : 1];
  if constexpr (M16) {
#pragma unroll
    for (int i = 0; i < 2 * TM; ++i)
#pragma unroll
      for (int j = 0; j < 2 * TN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc16[i][j][e] = 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  }

  const int kb_begin32 = sk ? seg_k0 : blockIdx.z * p.kb_per_split;
  const int kb_begin = kb_begin32 * (4 / KG);                       // in this kernel's k-blocks (16 or 32 k)
  // (the LAST split of a fused K-split tile -- its reducer -- takes whatever the others leave: the host may give them a
  // smaller share each, so that their partial tiles are in memory before the reducer is done with its own k-blocks)
  const int kb_end = (sk ? seg_k1 : ((int)blockIdx.z == (int)gridDim.z - 1 && p.sk_flags && p.partial)
                                        ? p.nkb : min(p.nkb, kb_begin32 + p.kb_per_split)) * (4 / KG);
  // Ring of NST stages.  In iteration kb the transfers of block kb+NST-1 are issued into the stage that was read in
  // iteration kb-1, the MFMAs run on stage kb%NST, then a COUNTED wait (all but the newest (NST-2)*NDMA transfers of
  // this wave, i.e. everything up to block kb+1) and a raw s_barrier publish stage (kb+1)%NST.  __syncthreads() would
  // drain vmcnt(0) and serialise the ~1-2 us L2/MALL -> LDS latency with every 0.3 us of MFMA work.
  KPos q;
  {   // k-block kb = (channel block, tap)
    const int taps = p.KH * p.KW;
    int cb = 0;
    q.ky = q.kx = 0;
    if (kb_begin32 != 0) {   // (a launch without K-split starts at k-block 0: no divisions)
      cb = kb_begin32 / taps;
      const int t = kb_begin32 - cb * taps;
      q.ky = t / p.KW;
      q.kx = t - q.ky * p.KW;
    }
    q.src = 0;
    int ci = cb * BK;
    if (ci >= p.c[0]) {
      ci -= p.c[0];
      q.src = 1;
      if (ci >= p.c[1]) {
        ci -= p.c[1];
        q.src = 2;
      }
    }
    q.ci0 = ci;
    set_src(q);
  }
  w_base = (unsigned)(kb_begin32 * 4 + g) * wgroup;
  set_tap(q);
  STAMP(1);
  // wait until at most `c` of this wave's k-block transfers (NDMA instructions each) are still in flight
  auto wait_blocks = [&](int c) __attribute__((always_inline)) {
    static_assert(3 * NDMA <= 63, "vmcnt is a 6-bit counter");
    if (c <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (c == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
    else if (c == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NDMA) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * NDMA) : "memory");
  };
  // The transfer of block kb+NST-1 is issued at the top of iteration kb, behind the previous iteration's MFMAs (NST-1 stages in
  // flight).  (Issuing it right behind the hand-over instead -- all NST stages in flight -- measured SLOWER: 308 against 330
  // TFLOP/s on 2x120x216 256->256, 296 against 338 on 2x30x54 1280->512: the eight waves' address work and transfer requests
  // right behind the barrier hold up all their MFMA chains at once.  The experiment's diff: profiles/r06_experiments/.)
  if constexpr (PF) {
    // ---------------------------------------------------------------------------------------------------------------
    // Prologue: all NST stages requested; block 0's fragments into register set 0; block 1 landed and published.
    issue(0);
    int issued = 1;
#pragma unroll
    for (int d = 1; d < NST; ++d)
      if (kb_begin + d < kb_end) {
        advance(q);
        issue(d);
        ++issued;
      }
    wait_blocks(issued - 1);
    __builtin_amdgcn_s_barrier();
    STAMP(2);
    const int r16 = lane & 15, kgl = lane >> 4;   // tile row / column, k/8 group of this lane
    const uint4 *Ab0 = As + kgl * SA + wm * 32 * TM + r16;
    const uint4 *Bb0 = Bs + kgl * SB + wn * 32 * TN + r16;
    uint4 fa[2][NPL][2 * TM], fb[2][NPL][2 * TN];
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
      for (int i = 0; i < 2 * TM; ++i) fa[0][pl][i] = Ab0[pl * PA + 16 * i];
#pragma unroll
      for (int i = 0; i < 2 * TN; ++i) fb[0][pl][i] = Bb0[pl * PB + 16 * i];
    }
    wait_blocks(issued - 2);
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the builtin, so that hipcc's own wait insertion knows the reads are done
    __builtin_amdgcn_s_barrier();
    int st = 0;   // stage of block kb: free from the top of iteration kb on (its fragments are in registers)
    STAMP_ACC_DECL(t_vm);
    STAMP_ACC_DECL(t_bar);
    auto body = [&](auto CUR, int kb) __attribute__((always_inline)) {
      constexpr int cur = decltype(CUR)::value, nxt = cur ^ 1;
      if (kb + NST < kb_end) {   // block kb+NST into the stage block kb occupied
        advance(q);
        issue(st);
      }
      const int stn = st == NST - 1 ? 0 : st + 1;   // stage of block kb+1: landed and published by the previous hand-over
      const bool more = kb + 1 < kb_end;
      const uint4 *Ab = Ab0 + stn * NPL * PA, *Bb = Bb0 + stn * NPL * PB;
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 2 * TM; ++i) {
        if (more) {   // this group's share of block kb+1's fragments: row tile i, and the column tiles dealt to it
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) {
            fa[nxt][pl][i] = Ab[pl * PA + 16 * i];
#pragma unroll
            for (int j = 0; j < 2 * TN; ++j)
              if (j * (2 * TM) / (2 * TN) == i) fb[nxt][pl][j] = Bb[pl * PB + 16 * j];
          }
        }
#pragma unroll
        for (int jn = 0; jn < 2 * TN; ++jn) {
          f32x4v c = acc16[i][jn];
          if constexpr (NPL >= 2) {   // "bf16x3": the three products above 2^-16, smallest first
            c = mm16<F16>(fa[cur][0][i], fb[cur][1][jn], c);
            c = mm16<F16>(fa[cur][1][i], fb[cur][0][jn], c);
          }
          c = mm16<F16>(fa[cur][0][i], fb[cur][0][jn], c);
          acc16[i][jn] = c;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (more) {
        // hand-over: this wave's share of block kb+2 has landed (the younger blocks may stay in flight), its reads of block
        // kb+1's stage are done; the barrier publishes the one and frees the other
        const int last = min(kb + NST, kb_end - 1);   // youngest block requested so far
        STAMP_T0(t_vm);
        if constexpr (NST == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else wait_blocks(last - (kb + 2));
        STAMP_ACC(t_vm);
        STAMP_T0(t_bar);
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the builtin, so that hipcc's own wait insertion knows the reads are done
        __builtin_amdgcn_s_barrier();
        STAMP_ACC(t_bar);
      }
      __builtin_amdgcn_sched_barrier(0);
      st = stn;
    };
    for (int kb = kb_begin; kb < kb_end; kb += 2) {
      body(std::integral_constant<int, 0>{}, kb);
      if (kb + 1 < kb_end) body(std::integral_constant<int, 1>{}, kb + 1);
    }
#ifndef SWEM_PROLOGUE_STAMPS
    STAMP_ACC_OUT(6, t_vm);
    STAMP_ACC_OUT(7, t_bar);
#endif
  } else {
    constexpr int NPRO = NST - 1;   // blocks issued before the loop
    issue(0);
    int issued = 1;   // k-blocks handed to the DMA so far (relative to kb_begin)
#pragma unroll
    for (int d = 1; d < NPRO; ++d)
      if (kb_begin + d < kb_end) {
        advance(q);
        issue(d);
        ++issued;
      }
    wait_blocks(issued - 1);   // block 0 has landed; the younger ones may stay in flight
    __builtin_amdgcn_s_barrier();
    STAMP(2);
    int st = 0;
    STAMP_ACC_DECL(t_vm);
    STAMP_ACC_DECL(t_bar);
    for (int kb = kb_begin; kb < kb_end; ++kb) {
      if (kb + NST - 1 < kb_end) {
        advance(q);
        issue(st == 0 ? NST - 1 : st - 1);  // stage (kb+NST-1) % NST
      }
      // Where the stage hand-over (counted wait for block kb+1 + s_barrier) sits inside the MFMA sequence: the MFMAs only
      // touch registers once the fragments are read, so any of them may run before or after it.  In front of it they would
      // hide the transfer this wave has just issued; behind it the waves of the block are decoupled while they compute (the
      // barrier does not wait for the slowest wave's MFMAs) and the next transfer starts earlier.  Measured on the config-B
      // layers (tools/conv_bench.py, tuned plans; none / half / all of the MFMAs in front): 330 / 334 / 310 TFLOP/s on
      // 2x120x216 256->256, 338 / 317 / 302 on 2x30x54 1280->512, 329 / 314 / 296 on 2x60x108 512->256 -- everything BEHIND the
      // hand-over wins: the other resident block's MFMAs hide the transfer, not this one's.  (The compiler's own scheduling had
      // arrived at nearly this order by sinking the MFMAs below the asm waits; it is now pinned by scheduling barriers.  The
      // two-waves-per-SIMD stagger and static-priority experiments of round 5 -- within +-1 % or 2-6 % slower -- are archived
      // with this one: profiles/r06_experiments/.)
      auto hand_over = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        // block kb+1 must have landed (this wave's share); the blocks behind it (up to kb+NST-1) may stay in flight
        const int last = min(kb + NST - 1, kb_end - 1);   // youngest block issued so far
        STAMP_T0(t_vm);
        wait_blocks(last - (kb + 1));
        STAMP_ACC(t_vm);
        STAMP_T0(t_bar);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's fragment reads of stage st are done
        __builtin_amdgcn_s_barrier();
        STAMP_ACC(t_bar);
        __builtin_amdgcn_sched_barrier(0);
      };
      if constexpr (M16) {
        const int r16 = lane & 15, kg = lane >> 4;   // tile row / column, k/8 group of this lane
        const uint4 *Ab = As + st * NPL * PA + kg * SA + wm * 32 * TM + r16;
        const uint4 *Bb = Bs + st * NPL * PB + kg * SB + wn * 32 * TN + r16;
        uint4 a[NPL][2 * TM], b[NPL][2 * TN];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
          for (int i = 0; i < 2 * TM; ++i) a[pl][i] = Ab[pl * PA + 16 * i];
#pragma unroll
          for (int i = 0; i < 2 * TN; ++i) b[pl][i] = Bb[pl * PB + 16 * i];
        }
#pragma unroll
        for (int i = 0; i < 2 * TM; ++i) {
          if (i == 0) hand_over();
#pragma unroll
          for (int jn = 0; jn < 2 * TN; ++jn) {
            f32x4v c = acc16[i][jn];
            if constexpr (NPL == 3) {
              c = mm16<F16>(a[0][i], b[2][jn], c);
              c = mm16<F16>(a[2][i], b[0][jn], c);
              c = mm16<F16>(a[1][i], b[1][jn], c);
            }
            if constexpr (NPL >= 2) {   // NPL == 2: "bf16x3", the three products above 2^-16
              c = mm16<F16>(a[0][i], b[1][jn], c);
              c = mm16<F16>(a[1][i], b[0][jn], c);
            }
            c = mm16<F16>(a[0][i], b[0][jn], c);
            acc16[i][jn] = c;
          }
        }
      } else {
        const uint4 *Ab = As + st * NPL * PA + wm * 32 * TM + r;
        const uint4 *Bb = Bs + st * NPL * PB + wn * 32 * TN + r;
        uint4 a[KG / 2][NPL][TM], b[KG / 2][NPL][TN];
#pragma unroll
        for (int s2 = 0; s2 < KG / 2; ++s2) {
          const int k8 = 2 * s2 + h;
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i) a[s2][pl][i] = Ab[pl * PA + k8 * SA + 32 * i];
#pragma unroll
            for (int i = 0; i < TN; ++i) b[s2][pl][i] = Bb[pl * PB + k8 * SB + 32 * i];
          }
        }
#pragma unroll
        for (int s2 = 0; s2 < KG / 2; ++s2) {
          if (s2 == 0) hand_over();
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int jn = 0; jn < TN; ++jn) {
              f32x16 c = acc[i][jn];
              if constexpr (NPL == 3) {
                c = mm32<F16>(a[s2][0][i], b[s2][2][jn], c);
                c = mm32<F16>(a[s2][2][i], b[s2][0][jn], c);
                c = mm32<F16>(a[s2][1][i], b[s2][1][jn], c);
              }
              if constexpr (NPL >= 2) {
                c = mm32<F16>(a[s2][0][i], b[s2][1][jn], c);
                c = mm32<F16>(a[s2][1][i], b[s2][0][jn], c);
              }
              c = mm32<F16>(a[s2][0][i], b[s2][0][jn], c);
              acc[i][jn] = c;
            }
        }
      }
      st = st == NST - 1 ? 0 : st + 1;
    }
#ifndef SWEM_PROLOGUE_STAMPS
    STAMP_ACC_OUT(6, t_vm);
    STAMP_ACC_OUT(7, t_bar);
#endif
  }
  STAMP(3);
  if (sk && (seg_k0 > 0 || seg_k1 < p.nkb)) {
    // the accumulators as 16-byte chunks per lane, chunk c of every lane contiguous (coalesced): the layout of a partial tile
    // (chunk c = accumulator tile c of the 16x16 layout, or quarter c % 4 of 32x32 tile c / 4: compile-time register indices)
    constexpr int NCH = 4 * TM * TN;   // float4 chunks per lane (16 accumulators per 32x32 of the wave tile)
    constexpr unsigned TILE_BYTES = BM * BN * 4;
    if (seg_k0 > 0) {   // a tile another worker began: hand the partial sums over, then go on
      const __amdgpu_buffer_rsrc_t rp =
          __builtin_amdgcn_make_buffer_rsrc(p.sk_ws + (long long)sk_v * (BM * BN), 0, TILE_BYTES, 0x00020000);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        u32x4 v;
        if constexpr (M16) {
          const f32x4v t = acc16[c / (2 * TN)][c % (2 * TN)];
          v.x = __float_as_uint(t[0]); v.y = __float_as_uint(t[1]); v.z = __float_as_uint(t[2]); v.w = __float_as_uint(t[3]);
        } else {
          const f32x16 t = acc[(c / 4) / TN][(c / 4) % TN];
          v.x = __float_as_uint(t[4 * (c % 4)]); v.y = __float_as_uint(t[4 * (c % 4) + 1]);
          v.z = __float_as_uint(t[4 * (c % 4) + 2]); v.w = __float_as_uint(t[4 * (c % 4) + 3]);
        }
        __builtin_amdgcn_raw_buffer_store_b128(v, rp, (unsigned)((c * 64 * NW + tid) * 16), 0, 0x11);   // sc0 sc1
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) __hip_atomic_store(p.sk_flags + sk_v, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    // the head of a tile: add the partial sums of the workers that hold the rest of it, in their order
    const long long tile_end = (long long)(sk_tile + 1) * p.nkb;
    for (int u = sk_v + 1; u < p.sk_workers; ++u) {
      if (sk_total * u / p.sk_workers >= tile_end) break;
      if (tid == 0) {
        int spins = 0;
        unsigned seen = __hip_atomic_load(p.sk_flags + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (seen == 0u && spins < p.spin_limit) {
          __builtin_amdgcn_s_sleep(16);
          ++spins;
          seen = __hip_atomic_load(p.sk_flags + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (seen == 0u && p.fault)   // the producer never arrived: what follows adds a tile that was not written
          __hip_atomic_fetch_or(p.fault, (unsigned)SWEM_FAULT_STREAMK_WAIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
      if (tid == 0) __hip_atomic_store(p.sk_flags + u, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // consumed once: leave it zero
      const __amdgpu_buffer_rsrc_t rp =
          __builtin_amdgcn_make_buffer_rsrc(p.sk_ws + (long long)u * (BM * BN), 0, TILE_BYTES, 0x00020000);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rp, (unsigned)((c * 64 * NW + tid) * 16), 0, 0x11);
        if constexpr (M16) {
          f32x4v t = acc16[c / (2 * TN)][c % (2 * TN)];
          t[0] += __uint_as_float(v.x); t[1] += __uint_as_float(v.y); t[2] += __uint_as_float(v.z); t[3] += __uint_as_float(v.w);
          acc16[c / (2 * TN)][c % (2 * TN)] = t;
        } else {
          f32x16 t = acc[(c / 4) / TN][(c / 4) % TN];
          t[4 * (c % 4)] += __uint_as_float(v.x); t[4 * (c % 4) + 1] += __uint_as_float(v.y);
          t[4 * (c % 4) + 2] += __uint_as_float(v.z); t[4 * (c % 4) + 3] += __uint_as_float(v.w);
          acc[(c / 4) / TN][(c / 4) % TN] = t;
        }
      }
    }
  }
  // ---- K-split without a reduce launch (round 3: p.sk_flags set, gridDim.z splits).  The LAST split (z = gridDim.z - 1) of a
  // tile is its reducer: the others store their partial tile past the caches (the stream-K layout: 16-byte chunks per lane),
  // drain, and count themselves on the tile's counter; the reducer keeps its own sums in registers, waits until the counter
  // says the others' tiles are in memory, adds them in z order (own + p0 + p1 + ...: a fixed order -- deterministic) and runs
  // the epilogue.  The reducer only ever waits for blocks dispatched BEFORE it (z is the slowest grid dimension), which are
  // resident or finished and wait for nobody: no deadlock whatever the grid size.  Against "the last arriver reduces"
  // (this round's first form) a tile's own sums never travel: 2 (nsp - 1) instead of 2 nsp tile moves -- the splits of a
  // layer finish together, so the stores and loads of the partials are a burst the matrix pipe cannot hide (13 of the 54 us
  // of `2x30x54 k3 512->512` at nsp = 4).  Replaces conv_splitk_epilogue_kernel for this kernel.
  bool fused_last = false;
  if constexpr (!SK) {
    if (p.partial && p.sk_flags) {
      constexpr int NCH = 4 * TM * TN;
      constexpr unsigned TILE_BYTES = BM * BN * 4;
      const int nsp = (int)gridDim.z, tile_lin = (tm - p.mt0) * (int)gridDim.y + tn;
      float *slots = p.partial + (long long)tile_lin * nsp * (BM * BN);
      if ((int)blockIdx.z != nsp - 1) {
        const __amdgpu_buffer_rsrc_t rp =
            __builtin_amdgcn_make_buffer_rsrc(slots + (long long)blockIdx.z * (BM * BN), 0, TILE_BYTES, 0x00020000);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          u32x4 v;
          if constexpr (M16) {
            const f32x4v t = acc16[c / (2 * TN)][c % (2 * TN)];
            v.x = __float_as_uint(t[0]); v.y = __float_as_uint(t[1]); v.z = __float_as_uint(t[2]); v.w = __float_as_uint(t[3]);
          } else {
            const f32x16 t = acc[(c / 4) / TN][(c / 4) % TN];
            v.x = __float_as_uint(t[4 * (c % 4)]); v.y = __float_as_uint(t[4 * (c % 4) + 1]);
            v.z = __float_as_uint(t[4 * (c % 4) + 2]); v.w = __float_as_uint(t[4 * (c % 4) + 3]);
          }
          __builtin_amdgcn_raw_buffer_store_b128(v, rp, (unsigned)((c * 64 * NW + tid) * 16), 0, 0x11);   // sc0 sc1
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(p.sk_flags + tile_lin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;   // not the reducer: done
      }
      fused_last = true;
      if (tid == 0) {
        // (a read-modify-write of zero: executed where the other splits' increments are, never served from a cache)
        // (>= and a bounded spin: a producer that is never dispatched -- XCDs advance their dispatch independently, so with
        // other streams' grids in flight the "dispatched before me" order is not a guarantee -- or counters left
        // non-zero by an aborted launch end in a wrong tile AND a set fault word, never in a hung queue)
        int spin = 0;
        unsigned seen = __hip_atomic_fetch_add(p.sk_flags + tile_lin, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (seen < (unsigned)(nsp - 1) && spin < p.spin_limit) {
          __builtin_amdgcn_s_sleep(8);
          ++spin;
          seen = __hip_atomic_fetch_add(p.sk_flags + tile_lin, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (seen < (unsigned)(nsp - 1) && p.fault)
          __hip_atomic_fetch_or(p.fault, (unsigned)SWEM_FAULT_KSPLIT_WAIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p.sk_flags + tile_lin, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // leave it zero
      }
      __syncthreads();
      for (int zz = 0; zz < nsp - 1; ++zz) {
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(slots + (long long)zz * (BM * BN), 0, TILE_BYTES, 0x00020000);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rp, (unsigned)((c * 64 * NW + tid) * 16), 0, 0x11);
          if constexpr (M16) {
            f32x4v t = acc16[c / (2 * TN)][c % (2 * TN)];
            t[0] += __uint_as_float(v.x); t[1] += __uint_as_float(v.y); t[2] += __uint_as_float(v.z); t[3] += __uint_as_float(v.w);
            acc16[c / (2 * TN)][c % (2 * TN)] = t;
          } else {
            f32x16 t = acc[(c / 4) / TN][(c / 4) % TN];
            t[4 * (c % 4)] += __uint_as_float(v.x); t[4 * (c % 4) + 1] += __uint_as_float(v.y);
            t[4 * (c % 4) + 2] += __uint_as_float(v.z); t[4 * (c % 4) + 3] += __uint_as_float(v.w);
            acc[(c / 4) / TN][(c / 4) % TN] = t;
          }
        }
      }
    }
  }
  if (fused_last) {   // the epilogue proper (the parameters' `partial` field only selects the raw-partials path)
    ConvP q = p;
    q.partial = nullptr;
    if constexpr (M16) conv_epilogue16<2 * TM, 2 * TN>(q, acc16, m0 + wm * 32 * TM, n0 + wn * 32 * TN, lane);
    else conv_epilogue<TM, TN>(q, acc, m0, n0, wm, wn, r, h);
  } else {
    if constexpr (M16) conv_epilogue16<2 * TM, 2 * TN>(p, acc16, m0 + wm * 32 * TM, n0 + wn * 32 * TN, lane);
    else conv_epilogue<TM, TN>(p, acc, m0, n0, wm, wn, r, h);
  }
  STAMP(4);
  if (!sk) break;
  }   // segments
#ifdef SWEM_EM_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  STAMP(5);
#endif
}

// resident blocks per CU of one instantiation at its dynamic-LDS size (stream-K sizes its persistent grid by it): the
// runtime's occupancy figure, never more than the LDS allows (the API has been seen one block per CU high near SGPR-count
// edges, MI355X_MICROARCH.md: an over-sized persistent grid only costs a second, short round here -- no worker ever waits
// on a worker that has not produced its partial sums first -- but the balance is lost)
template <typename K>
int blocks_per_cu(K kernel, int threads, size_t lds) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(kernel), threads, lds) != hipSuccess || nb < 1)
    nb = 1;
  const int by_lds = (int)((160 * 1024) / (lds ? lds : 1));
  if (by_lds >= 1 && nb > by_lds) nb = by_lds;
  const int by_waves = 32 / (threads / 64);
  return nb > by_waves ? by_waves : nb;
}

// occ != nullptr: do not launch, report the resident blocks per CU of the instantiation the launch would use
// (p.sk_workers != 0 selects the stream-K instantiation: a query passes -1)
template <int WM, int WN, int NST, int NW, bool M16, int KG, bool PF, int NPL, bool SK, bool F16 = false>
int launch_bf3s_one(const ConvP &p, dim3 grid, hipStream_t st, int *occ) {
  constexpr size_t lds = NST * NPL * KG * (64 * WM + 1 + 64 * WN + 1) * 16;   // NST stages x NPL planes
  const size_t dyn = lds_with_planes(p, lds, NW);
  SWEM_ALLOW_LDS((conv_igemm_bf3s_kernel<WM, WN, NST, NW, M16, NPL, KG, PF, SK, F16>), lds);
  if (occ) {
    // (asked anew on every query: the answer depends on the instantiation, its dynamic-LDS size and the current device, and a
    // cached copy would be unsynchronised mutable state in a library whose contract is "re-entrant across streams" -- the
    // query costs microseconds and only stream-K launches make it)
    *occ = blocks_per_cu(conv_igemm_bf3s_kernel<WM, WN, NST, NW, M16, NPL, KG, PF, SK, F16>, 64 * NW, dyn);
    return SWEM_OK;
  }
  hipLaunchKernelGGL((conv_igemm_bf3s_kernel<WM, WN, NST, NW, M16, NPL, KG, PF, SK, F16>), grid, dim3(64 * NW), dyn, st, p STAMP_PASS);
  return SWEM_OK;
}
template <int WM, int WN, int NST, int NW, bool M16 = false, int KG = 4, bool PF = false>
int launch_bf3s_n(const ConvP &p, dim3 grid, hipStream_t st, int *occ = nullptr) {
  const bool sk = p.sk_workers != 0;
  // stream-K instantiations exist for the two-plane ("bf16x3") and one-plane kernels of the eight-wave 16x16x32 tile and of
  // the prefetched-fragment tiles (what the tuner is offered); everything else runs the plain grid
  constexpr bool SKOK = M16 && KG == 4 && NST == 2 && (NW == 8 || PF);
  if (sk && !(SKOK && p.nplanes <= 2)) {
    if (occ) {
      *occ = 0;   // no stream-K form of this variant: the caller launches the plain grid
      return SWEM_OK;
    }
    swem_set_error("conv2d_bf16x3: this kernel variant has no stream-K form");
    return SWEM_E_ARG;
  }
  // (SWEM_ISA_SUBSET: tests/test_abi.py compiles this unit to assembly to check the LDS-DMA kernels' use of M0; a fifth of the
  // instantiations -- every tile, the two-plane kernels of both operand formats, no stream-K -- keeps that check to a minute)
#ifndef SWEM_ISA_SUBSET
  if (p.nplanes == 1) {   // plain bf16 (one plane, one product): a third of the LDS, the same tiles
    if constexpr (SKOK) {
      if (sk) return launch_bf3s_one<WM, WN, NST, NW, M16, KG, PF, 1, true>(p, grid, st, occ);
    }
    return launch_bf3s_one<WM, WN, NST, NW, M16, KG, PF, 1, false>(p, grid, st, occ);
  }
#endif
  if (p.nplanes == 2 && p.f16) {   // "f16x3": the same kernel on fp16 (hi, mid) planes and the f16 MFMA
    if (sk) {
      if (occ) {
        *occ = 0;
        return SWEM_OK;
      }
      swem_set_error("conv2d_bf16x3: the f16x3 arithmetic has no stream-K form");
      return SWEM_E_ARG;
    }
    return launch_bf3s_one<WM, WN, NST, NW, M16, KG, PF, 2, false, true>(p, grid, st, occ);
  }
  if (p.nplanes == 2) {   // "bf16x3": hi and mid planes, three products (hi.hi + hi.mid + mid.hi): two thirds of the LDS
#ifndef SWEM_ISA_SUBSET
    if constexpr (SKOK) {
      if (sk) return launch_bf3s_one<WM, WN, NST, NW, M16, KG, PF, 2, true>(p, grid, st, occ);
    }
#endif
    return launch_bf3s_one<WM, WN, NST, NW, M16, KG, PF, 2, false>(p, grid, st, occ);
  }
#ifndef SWEM_ISA_SUBSET
  if constexpr (NST <= 3 && !PF) {
    return launch_bf3s_one<WM, WN, NST, NW, M16, KG, PF, 3, false>(p, grid, st, occ);
  }
#endif
  swem_set_error("conv2d_bf16x3: four-stage rings and prefetched fragments need at most two planes");
  return SWEM_E_ARG;
}

// variant (plan bits 20-23): 0 = the tile's default; 1 = three LDS stages instead of two (or two instead of three);
// 2 = eight waves on the 128x128 tile (two stages), 3 = eight waves, three stages; 4 / 6 = variants 0 / 2 on the
// 16x16x32 MFMA shape
template <int WM, int WN>
int launch_bf3s(const ConvP &p, dim3 grid, hipStream_t st, int variant, int *occ = nullptr) {
  // deeper rings (round 2): with two planes a stage is 33 KB for the 128x128 tile, so FOUR stages fit; the k-loop of every
  // tile was bound by the L2 / Infinity-Cache -> LDS latency of the one or two k-blocks in flight (in-kernel stamps,
  // tools/conv_stamps.py: 2600 cycles per k-block against 768 of MFMA on the 128x128 tile, 830 against 192 on 64x64)
#ifndef SWEM_ISA_SUBSET
  if (p.nplanes <= 2) {
    if constexpr (WM == 2 && WN == 2) {
      if (variant == 12) return launch_bf3s_n<2, 2, 4, 8>(p, grid, st, occ);
      if (variant == 13) return launch_bf3s_n<2, 2, 4, 8, true>(p, grid, st, occ);
    }
    if constexpr (WM == 2 && WN == 2) {
      // prefetched fragments (PF): 5 = four waves of 64x64, two stages (two blocks per CU); 15 = four waves, three stages (one
      // block per CU, one wave per SIMD); 7 = eight waves of 32x64, four stages (one block per CU)
      if (variant == 5) return launch_bf3s_n<2, 2, 2, 4, true, 4, true>(p, grid, st, occ);
      if (variant == 15) return launch_bf3s_n<2, 2, 3, 4, true, 4, true>(p, grid, st, occ);
      if (variant == 7) return launch_bf3s_n<2, 2, 4, 8, true, 4, true>(p, grid, st, occ);
    }
    if (variant == 10) return launch_bf3s_n<WM, WN, 4, 4>(p, grid, st, occ);
    if (variant == 11) return launch_bf3s_n<WM, WN, 4, 4, true>(p, grid, st, occ);
  }
#endif
  if constexpr (WM == 2 && WN == 2) {
#ifndef SWEM_ISA_SUBSET
    if (variant == 14) return launch_bf3s_n<2, 2, 3, 8, true>(p, grid, st, occ);
    if (variant == 2) return launch_bf3s_n<2, 2, 2, 8>(p, grid, st, occ);
    if (variant == 3) return launch_bf3s_n<2, 2, 3, 8>(p, grid, st, occ);
    if (variant == 9) return launch_bf3s_n<2, 2, 3, 4, false, 2>(p, grid, st, occ);   // ... three stages: two blocks per CU
#endif
    if (variant == 6) return launch_bf3s_n<2, 2, 2, 8, true>(p, grid, st, occ);
    if (variant == 8) return launch_bf3s_n<2, 2, 2, 4, false, 2>(p, grid, st, occ);   // 16-k blocks: three blocks per CU
  }
  if (variant == 4)
    return (WM * WN == 1) ? launch_bf3s_n<WM, WN, 3, 4, true>(p, grid, st, occ) : launch_bf3s_n<WM, WN, 2, 4, true>(p, grid, st, occ);
  const bool three = (WM * WN == 1) != (variant == 1);
  return three ? launch_bf3s_n<WM, WN, 3, 4>(p, grid, st, occ) : launch_bf3s_n<WM, WN, 2, 4>(p, grid, st, occ);
}

}  // namespace

int swem_conv_presplit_launch(const ConvP &p, int wm, int wn, int variant, dim3 grid, hipStream_t st, int *occ) {
  if (wm == 2 && wn == 2) return launch_bf3s<2, 2>(p, grid, st, variant, occ);
  if (wm == 1 && wn == 2) return launch_bf3s<1, 2>(p, grid, st, variant, occ);
  if (wm == 2 && wn == 1) return launch_bf3s<2, 1>(p, grid, st, variant, occ);   // 128x64: the 64-channel layers
  return launch_bf3s<1, 1>(p, grid, st, variant, occ);
}
