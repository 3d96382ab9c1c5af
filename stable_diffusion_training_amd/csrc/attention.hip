// Exact softmax attention (flash-style, no N x N materialisation) for gfx950, forward and backward.
// Replaces diffusers 0.21.4 attention_flax.jax_memory_efficient_attention as patched by
// key_chunk_patch.patch:1-9 (key chunk == all keys => plain exact softmax(q k^T / sqrt(d)) v, computed
// query-block by query-block), its transpose under jax.value_and_grad (training_utils.py:719-729), and the
// causal self-attention of transformers FlaxCLIPTextModel (training_utils.py:635-640).
//
// Layout: q/k/v/o are (B, N, H*D) row-major bf16 with explicit row strides; a head is the D-wide column
// slice h*D.. (no head transposes are ever materialised).  lse is (B, H, Nq) fp32 in the log2 domain:
// lse2 = max2 + log2(sum exp2(s2 - max2)), s2 = q.k * scale * log2(e).
//
// MFMA mapping (v_mfma_f32_32x32x16_bf16, one wave = 32 queries or 32 keys on the lanes):
//   fwd / dq : S^T = K Q^T   (keys on accumulator rows, query on the lane => row max / sum / LSE are per-lane
//              scalars, and the bf16-converted accumulator is directly the B operand of the next product)
//              O^T += V^T P^T,   dP^T = V dO^T,   dQ^T += K^T dS^T
//   dkv      : S = Q K^T, dP = dO V^T (key on the lane), dV^T += dO^T P, dK^T += Q^T dS
//
// Staging: every 64-token tile of K/V (fwd, dq) or Q/dO (dkv) is copied global -> LDS by the LDS-DMA path
// (global_load_lds, 16 B per lane, no VGPR round trip) into ONE row-major image [64 tokens][DPP features] per
// tensor, double buffered so tile t+1 lands while tile t is in the MFMAs (one barrier per tile).  Both operand
// shapes are read from that image: [token][feature] fragments with ds_read_b128, and the transposed
// [feature][token] fragments with ds_read_b64_tr_b16.  The k-order of an accumulator-as-operand step is permuted
// (element j of lane half h is accumulator row 16s + 8(j>>2) + 4h + (j&3)), so the transposed fragment is two
// tr reads at token rows 16s+4h.. and 16s+8+4h...  Padding (features >= D, tokens >= N) is DMA'd from a zero page.
// The 16-byte chunks of a row are XOR-swizzled on the SOURCE side (LDS-DMA writes lane-linear) so that both read
// shapes are bank-conflict free.
#include <type_traits>

#include "sdt_common.h"

#define KT 64  // keys (or queries) staged per LDS tile
#define NEG_BIG -1.0e30f

typedef __attribute__((ext_vector_type(4))) short s16x4_t;

__device__ __attribute__((aligned(16))) unsigned int g_attn_zero16[4] = {0u, 0u, 0u, 0u};
// bf16 {1, 0, 0, 0, 0, 0, 0, 0}: the chunk that turns one padded V feature into a column of ones, so that the P.V
// MFMAs also deliver the softmax row sum (forward kernel, head dims with spare padding)
__device__ __attribute__((aligned(16))) unsigned int g_attn_one16[4] = {0x3f80u, 0u, 0u, 0u};

// LDS-DMA, asm-owned.  hipcc treats an in-flight global_load_lds as a pending LDS write and drains it (s_waitcnt vmcnt(0)) in front
// of the first LDS read it can see behind it - in the dK/dV loop that is the top of the tile body, so every wave sat out the whole
// flight of the NEXT tile's DMA before it touched the current one.  A DMA the compiler cannot see is ordered by hand instead:
// dma_join() (vmcnt(0), then the barrier) before any read of the image it fills.  M0 carries the wave's LDS destination and is
// restored; lds_wave_base must be wave-uniform.  (hipcc's own vmcnt(N) for its loads stays safe: the counter retires in order and
// extra younger operations only make such a wait longer.)
__device__ __forceinline__ unsigned lds_offset_of(const void* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char*)p;
}
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_offset_of(lds_wave_base)) : "memory");
}
__device__ __forceinline__ void glds4(const void* gsrc, void* lds_wave_base) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_offset_of(lds_wave_base)) : "memory");
}

__device__ __forceinline__ bf16x8_t cvt_frag(const float* p) {
  uint4 u;
  u.x = pack2bf(p[0], p[1]); u.y = pack2bf(p[2], p[3]); u.z = pack2bf(p[4], p[5]); u.w = pack2bf(p[6], p[7]);
  return __builtin_bit_cast(bf16x8_t, u);
}

// One staged image: [KT rows][DPP features] bf16, DPP in {64, 128, 256} (row = 128 / 256 / 512 bytes).
template <int DPP>
struct Img {
  static constexpr int RB = DPP * 2;            // bytes per row
  static constexpr int CPR = DPP / 8;           // 16-byte chunks per row
  static constexpr int BYTES = KT * RB;
  static constexpr int IPW = BYTES / 1024 / 4;  // LDS-DMA instructions per wave per image
  // chunk XOR of a row: 16 consecutive rows at one chunk (b128 fragment reads) and 4 consecutive rows x 4 chunks
  // (tr reads of one 32-lane half) both cover all 16 slots of the 256-byte bank window exactly once
  static __device__ __forceinline__ int swz(int row) {
    if (CPR == 8) return (((row >> 1) & 1) << 2) | ((row >> 2) & 3);
    return ((row & 3) << 2) | ((row >> 2) & 3);
  }
};

// per-lane source map of the image DMA: instruction i of wave w fills LDS bytes [(w*IPW+i)*1024, +1024)
template <int DPP>
struct TileDma {
  static constexpr int IPW = Img<DPP>::IPW, CPR = Img<DPP>::CPR;
  int row[IPW];  // token row inside the tile
  int col[IPW];  // first feature of the lane's chunk, -1 when it lies in the zero padding, -2 for the ones chunk (init's ones_chunk)
  __device__ __forceinline__ void init(int wave, int lane, int D, int ones_chunk = -1) {
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      const int L = (wave * IPW + i) * 64 + lane;
      const int r = L / CPR, slot = L % CPR;
      const int c = slot ^ Img<DPP>::swz(r);
      row[i] = r;
      col[i] = (c * 8 < D) ? c * 8 : (c == ones_chunk ? -2 : -1);
    }
  }
  // Tiles are issued in token order, KT apart: the lane's source pointers are kept and ADVANCED instead of being rebuilt from
  // (token, stride, column) every tile.  Which source a piece has - a real column, the zero page or the ones chunk - is known at
  // bind(): a padded lane's pointer stands at its page and never moves, so a full tile (every tile but a tensor's ragged last one)
  // is one DMA and one pointer add per piece, with no selects - the attention loops are VALU-issue bound and the per-tile source
  // selection was a quarter of the forward's vector instructions.
  const bf16_t* ptr[IPW];
  unsigned step;  // bytes per tile (KT rows); pointers at a page do not advance
  // src: the (batch, head) base of the tensor; tok0: first token of the first tile that will be issued
  __device__ __forceinline__ void bind(const bf16_t* src, long ld, int tok0) {
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      const bf16_t* page = reinterpret_cast<const bf16_t*>(col[i] == -2 ? g_attn_one16 : g_attn_zero16);
      ptr[i] = col[i] >= 0 ? src + ((long)(tok0 + row[i]) * ld + col[i]) : page;
    }
    step = (unsigned)(KT * ld * sizeof(bf16_t));
  }
  // issues the tile the pointers stand at (its first token is tok_base: only the ragged tile's bounds test uses it) and advances
  // them; img: wave-uniform image base.  Rows past the tensor's end come from the zero page (the ones column included).
  __device__ __forceinline__ void issue(int tok_base, int ntok, unsigned char* img, int wave_u) {
    if (tok_base + KT <= ntok) {  // wave-uniform
#pragma unroll
      for (int i = 0; i < IPW; ++i) glds16(ptr[i], img + (wave_u * IPW + i) * 1024);
    } else {
      const bf16_t* zero = reinterpret_cast<const bf16_t*>(g_attn_zero16);
#pragma unroll
      for (int i = 0; i < IPW; ++i) glds16(tok_base + row[i] < ntok ? ptr[i] : zero, img + (wave_u * IPW + i) * 1024);
    }
#pragma unroll
    for (int i = 0; i < IPW; ++i)
      ptr[i] = reinterpret_cast<const bf16_t*>(reinterpret_cast<const unsigned char*>(ptr[i]) + (col[i] >= 0 ? step : 0u));
  }
};

// [token][feature] fragment: 8 features (chunk) of one token row
template <int DPP>
__device__ __forceinline__ bf16x8_t row_frag(const unsigned char* img, int row, int chunk) {
  return *reinterpret_cast<const bf16x8_t*>(img + row * Img<DPP>::RB + ((chunk ^ Img<DPP>::swz(row)) << 4));
}

// per-lane constants of the transposed fragment reads
template <int DPP>
struct TrLane {
  int off1, off2;  // byte offset of the lane's row (tile-local 4h+q, +8) with the `within` part folded in
  int cx1, cx2;    // (lane chunk) ^ swz(row)
  __device__ __forceinline__ void init(int lane) {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int r1 = 4 * (g >> 1) + q, r2 = r1 + 8;
    const int cl = 2 * (g & 1) + (pp >> 1), within = (pp & 1) * 8;
    off1 = r1 * Img<DPP>::RB + within;
    off2 = r2 * Img<DPP>::RB + within;
    cx1 = cl ^ Img<DPP>::swz(r1);
    cx2 = cl ^ Img<DPP>::swz(r2);
  }
  // A operand [32 features fb*32.. on the lanes][16 tokens tok0.. as k, accumulator-permuted order]; tok0 % 16 == 0
  __device__ __forceinline__ bf16x8_t frag(const unsigned char* img, int tok0, int fb) const {
    const unsigned char* a1 = img + tok0 * Img<DPP>::RB + off1 + (((fb * 4) ^ cx1) << 4);
    const unsigned char* a2 = img + tok0 * Img<DPP>::RB + off2 + (((fb * 4) ^ cx2) << 4);
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)a1);
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)a2);
    bf16x8_t f;
    f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3]; f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
    return f;
  }
};

// all of this wave's LDS-DMA has landed, then every wave's (the barrier); also closes the reads of the previous tile.
// The asm wait is the one that counts (the DMA is asm-owned).  The builtin behind it is for hipcc's own bookkeeping: it drops it
// where it has no load of its own in flight, and otherwise learns here that its loads (the Q / K fragments fetched ahead of the loop,
// key weights) have landed - without it, it waits for them with a vmcnt(0) of its own INSIDE the tile body, behind the issue of the
// next tile's DMA, on every tile.
__device__ __forceinline__ void dma_join() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), nothing else
  __syncthreads();
}

struct AttnParams {
  const bf16_t *q, *k, *v, *o, *dout;
  bf16_t *out, *dq, *dk, *dv;
  float* lse;          // (B,H,Nq) log2 domain
  const float* delta;  // (B,H,Nq)
  int B, H, Nq, Nk, D;
  long ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;  // row strides (elements)
  long bsq, bsk, bsv, bso, bsdo, bsdq, bsdk, bsdv;  // batch strides (elements)
  float scale2;  // scale * log2(e)
  float scale;
  int causal;
  // dK/dV with the query range split over workgroups (few keys, many queries: cross-attention): each query chunk writes its partial
  // sums to its own fp32 slab [2][B][Nk][H*D] and attn_kv_finish_kernel adds the slabs in order and rounds them into dk / dv
  float* kv_ws;
  int qchunk, kblocks;
  // optional per-key weights w[Nk] > 0: P = softmax(s + ln w).  Emulates the key chunks of diffusers' memory-efficient attention,
  // whose last chunk is a clamped (overlapping) slice when the key count is not a multiple of the chunk: overlapped keys count twice
  const float* key_w;
};

// Runs the tile loop `tiles(masked, weighted, from, to)` over the tiles [from, to) of a tensor of n tokens (tile starts from + j * KT)
// with the wave-uniform choice of the body made OUTSIDE the loop: key weights -> the masked, weighted body; always_mask (causal, or
// a ragged block on the other axis) -> the masked body; otherwise the full tiles run the plain body and only the ragged last tile
// the masked one.  Choosing per tile inside one loop made the accumulators phis of three bodies, which hipcc resolved with a second
// copy of them (32 - 64 registers) and a register move per accumulator and tile.
template <typename F>
__device__ __forceinline__ void attn_tile_loops(F& tiles, bool weighted, bool always_mask, int from, int to, int n) {
  if (weighted) {
    tiles(std::true_type{}, std::true_type{}, from, to);  // (cross-attention with repeated text keys: few, small tiles)
  } else {
    const int split = always_mask ? from : min(to, from + (n > from ? (n - from) / KT * KT : 0));  // first tile that is not full
    tiles(std::false_type{}, std::false_type{}, from, split);
    tiles(std::true_type{}, std::false_type{}, split, to);
  }
}

// ------------------------------------------------------------------------------------------ forward
// DPP: image pitch (features); NS = ceil(D/16) k-steps of q.k; NB = ceil(D/32) feature blocks of the output.
// MSUM: D <= NB*32 - 8, so V's padded feature NB*32-8 is staged as a column of ones and the softmax denominator is
// accumulated by the P.V MFMAs themselves (accumulator row 24 of the last block = register 12 of lanes 0..31).
// The running max is only raised when some row's maximum grew by more than 2^RESCALE_LOG2 (probabilities then stay below
// that bound instead of 1, which fp32 accumulation and the scale-free bf16 rounding of P do not notice), so most tiles skip
// the rescale of the output accumulators.
#define RESCALE_LOG2 8.0f
template <int DPP, int NS, int NB, bool MSUM>
__global__ void __launch_bounds__(256) attn_fwd_kernel(const AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using I = Img<DPP>;
  constexpr int STAGE = 2 * I::BYTES;  // K image | V image
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * 128;
  const int qi = q0 + wave * 32 + fr;  // this lane's query
  const bf16_t* qb = p.q + (long)b * p.bsq + h * p.D;
  const bf16_t* kb = p.k + (long)b * p.bsk + h * p.D;
  const bf16_t* vb = p.v + (long)b * p.bsv + h * p.D;

  TileDma<DPP> dma, dmav;
  dma.init(wave, lane, p.D);
  dmav.init(wave, lane, p.D, MSUM ? NB * 4 - 1 : -1);
  TrLane<DPP> tr;
  tr.init(lane);
  int kend = p.Nk;
  if (p.causal) kend = min(p.Nk, q0 + 128);  // keys beyond the block's last query are fully masked
  dma.bind(kb, p.ldk, 0);
  dmav.bind(vb, p.ldv, 0);
  dma.issue(0, p.Nk, smem, wave_u);
  dmav.issue(0, p.Nk, smem + I::BYTES, wave_u);

  bf16x8_t qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    uint4 v = make_uint4(0, 0, 0, 0);
    const int d0 = 16 * s + 8 * fh;
    if (qi < p.Nq && d0 < p.D) v = *reinterpret_cast<const uint4*>(qb + (long)qi * p.ldq + d0);
    qf[s] = __builtin_bit_cast(bf16x8_t, v);
  }
  f32x16_t o_acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) o_acc[i][e] = 0.f;
  float m_run = NEG_BIG, l_run = 0.f;
  int cur = 0;
  // One tile LOOP per straight-line body, the wave-uniform choice (mask, key weights) made outside it (attn_tile_loops): a test
  // between the exponentials and the P.V products ends the basic block there and nothing is scheduled across it - no MFMA ran
  // beside the softmax.
  auto tiles = [&](auto masked, auto weighted, int kfrom, int kto) {
    constexpr bool MASK = decltype(masked)::value, KW = decltype(weighted)::value;
    for (int kbase = kfrom; kbase < kto; kbase += KT, cur ^= 1) {
      dma_join();
      if (kbase + KT < kend) {  // next tile flies under this tile's math
        dma.issue(kbase + KT, p.Nk, smem + (cur ^ 1) * STAGE, wave_u);
        dmav.issue(kbase + KT, p.Nk, smem + (cur ^ 1) * STAGE + I::BYTES, wave_u);
      }
      const unsigned char* k_img = smem + cur * STAGE;
      const unsigned char* v_img = k_img + I::BYTES;
      f32x16_t st[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) st[kt][e] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bf16x8_t kf = row_frag<DPP>(k_img, kt * 32 + fr, 2 * s + fh);
          st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], st[kt], 0, 0, 0);
        }
      }
      // running max on the RAW scores (scale2 > 0), scale folded into the exp2 argument; masks only where needed
      float mx = NEG_BIG;
      if (MASK) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = kbase + kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
            if (key >= p.Nk || (p.causal && key > qi)) st[kt][e] = NEG_BIG;
          }
      }
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, st[kt][e]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      if (__any((mx - m_run) * p.scale2 > RESCALE_LOG2)) {  // wave-uniform; always taken on the first tile (m_run = -big)
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.scale2);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) o_acc[i][e] *= alpha;
      }
      const float mneg = -m_run * p.scale2;
      float kwv[2][16];
      if (KW) {  // the running max stays on the unweighted scores (weights are O(1)); one batch of loads ahead of the exponentials
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = kbase + kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
            kwv[kt][e] = p.key_w[min(key, p.Nk - 1)];
          }
      }
      // P = exp2(...) and O^T += V^T P^T, eight keys (one k-step of the product) at a time: the products of one group run
      // beside the exponentials of the next
      float psum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float tmp[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int e = 8 * s + j;
            float pv = __builtin_amdgcn_exp2f(fmaf(st[kt][e], p.scale2, mneg));
            if (KW) pv *= kwv[kt][e];
            if (!MSUM) psum += pv;
            tmp[j] = pv;
          }
          const bf16x8_t pf = cvt_frag(tmp);
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const bf16x8_t vf = tr.frag(v_img, kt * 32 + 16 * s, i);
            o_acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o_acc[i], 0, 0, 0);
          }
          // groups stay in program order: the matrix pipe works through this group's products while the next group's
          // exponentials issue; left free, hipcc hoists every group's V reads and exponentials to the top (+40 registers)
          __builtin_amdgcn_sched_barrier(0);
        }
      if (!MSUM) l_run += psum;
    }
  };
  attn_tile_loops(tiles, p.key_w != nullptr, p.causal != 0, 0, kend, p.Nk);
  float l_tot;
  if (MSUM) l_tot = __shfl(o_acc[NB - 1][12], fr, 64);  // ones-column row sum: accumulator row 24 lives in lanes 0..31
  else l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv_l = 1.f / l_tot;
  if (qi < p.Nq) {
    if (fh == 0 && p.lse) p.lse[((long)b * p.H + h) * p.Nq + qi] = m_run * p.scale2 + log2f(l_tot);
    bf16_t* ob = p.out + (long)b * p.bso + (long)qi * p.ldo + h * p.D;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = i * 32 + 8 * g4 + 4 * fh;
        if (d < p.D) {
          uint2 pk;
          pk.x = pack2bf(o_acc[i][4 * g4] * inv_l, o_acc[i][4 * g4 + 1] * inv_l);
          pk.y = pack2bf(o_acc[i][4 * g4 + 2] * inv_l, o_acc[i][4 * g4 + 3] * inv_l);
          *reinterpret_cast<uint2*>(ob + d) = pk;
        }
      }
  }
}

// ------------------------------------------------------------------------------------------ backward: dQ
template <int DPP, int NS, int NB>
__global__ void __launch_bounds__(256) attn_bwd_dq_kernel(const AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using I = Img<DPP>;
  constexpr int STAGE = 2 * I::BYTES;  // K image | V image
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * 128;
  const int qi = q0 + wave * 32 + fr;
  const bf16_t* qb = p.q + (long)b * p.bsq + h * p.D;
  const bf16_t* dob = p.dout + (long)b * p.bsdo + h * p.D;
  const bf16_t* kb = p.k + (long)b * p.bsk + h * p.D;
  const bf16_t* vb = p.v + (long)b * p.bsv + h * p.D;

  TileDma<DPP> dma, dmav;
  dma.init(wave, lane, p.D);
  dmav.init(wave, lane, p.D);
  TrLane<DPP> tr;
  tr.init(lane);
  int kend = p.Nk;
  if (p.causal) kend = min(p.Nk, q0 + 128);
  dma.bind(kb, p.ldk, 0);
  dmav.bind(vb, p.ldv, 0);
  dma.issue(0, p.Nk, smem, wave_u);
  dmav.issue(0, p.Nk, smem + I::BYTES, wave_u);

  bf16x8_t qf[NS], dof[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    uint4 v = make_uint4(0, 0, 0, 0), w = make_uint4(0, 0, 0, 0);
    const int d0 = 16 * s + 8 * fh;
    if (qi < p.Nq && d0 < p.D) {
      v = *reinterpret_cast<const uint4*>(qb + (long)qi * p.ldq + d0);
      w = *reinterpret_cast<const uint4*>(dob + (long)qi * p.lddo + d0);
    }
    qf[s] = __builtin_bit_cast(bf16x8_t, v);
    dof[s] = __builtin_bit_cast(bf16x8_t, w);
  }
  // delta[q] = sum_d dO[q][d] * O[q][d]: each lane already holds half of its query's dO row, so the dq kernel computes the
  // row dot itself and publishes it for the dK/dV kernel launched behind it (no separate pass over dO and O)
  float lse2 = 0.f, dlt = 0.f;
  if (qi < p.Nq) {
    lse2 = p.lse[((long)b * p.H + h) * p.Nq + qi];
    const bf16_t* orow = p.o + (long)b * p.bso + (long)qi * p.ldo + h * p.D;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int d0 = 16 * s + 8 * fh;
      if (d0 < p.D) {
        float fo[8], fd[8];
        unpack8(*reinterpret_cast<const uint4*>(orow + d0), fo);
        unpack8(__builtin_bit_cast(uint4, dof[s]), fd);
#pragma unroll
        for (int e = 0; e < 8; ++e) dlt += fo[e] * fd[e];
      }
    }
  }
  dlt += __shfl_xor(dlt, 32, 64);
  if (qi < p.Nq && fh == 0) const_cast<float*>(p.delta)[((long)b * p.H + h) * p.Nq + qi] = dlt;
  f32x16_t dq_acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) dq_acc[i][e] = 0.f;

  int cur = 0;
  // straight-line tile bodies, one loop each (attn_tile_loops; see attn_bwd_dkv_kernel)
  auto tiles = [&](auto masked, auto weighted, int kfrom, int kto) {
    constexpr bool MASK = decltype(masked)::value, KW = decltype(weighted)::value;
    for (int kbase = kfrom; kbase < kto; kbase += KT, cur ^= 1) {
      dma_join();
      if (kbase + KT < kend) {
        dma.issue(kbase + KT, p.Nk, smem + (cur ^ 1) * STAGE, wave_u);
        dmav.issue(kbase + KT, p.Nk, smem + (cur ^ 1) * STAGE + I::BYTES, wave_u);
      }
      const unsigned char* k_img = smem + cur * STAGE;
      const unsigned char* v_img = k_img + I::BYTES;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        f32x16_t st, dpt;
#pragma unroll
        for (int e = 0; e < 16; ++e) { st[e] = 0.f; dpt[e] = -dlt; }  // dP - delta comes out of the MFMA chain
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bf16x8_t kf = row_frag<DPP>(k_img, kt * 32 + fr, 2 * s + fh);
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], st, 0, 0, 0);
          const bf16x8_t vf = row_frag<DPP>(v_img, kt * 32 + fr, 2 * s + fh);
          dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[s], dpt, 0, 0, 0);
        }
        float ds[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float pv = __builtin_amdgcn_exp2f(fmaf(st[e], p.scale2, -lse2));
          const int key = kbase + kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
          if (MASK) pv = (key >= p.Nk || (p.causal && key > qi) || qi >= p.Nq) ? 0.f : pv;
          if (KW) pv *= p.key_w[min(key, p.Nk - 1)];
          ds[e] = pv * dpt[e];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8_t dsf = cvt_frag(ds + 8 * s);
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const bf16x8_t ktf = tr.frag(k_img, kt * 32 + 16 * s, i);
            dq_acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf, dsf, dq_acc[i], 0, 0, 0);
          }
        }
      }
    }
  };
  attn_tile_loops(tiles, p.key_w != nullptr, p.causal || q0 + 128 > p.Nq, 0, kend, p.Nk);
  if (qi < p.Nq) {
    bf16_t* ob = p.dq + (long)b * p.bsdq + (long)qi * p.lddq + h * p.D;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = i * 32 + 8 * g4 + 4 * fh;
        if (d < p.D) {
          uint2 pk;
          pk.x = pack2bf(dq_acc[i][4 * g4] * p.scale, dq_acc[i][4 * g4 + 1] * p.scale);
          pk.y = pack2bf(dq_acc[i][4 * g4 + 2] * p.scale, dq_acc[i][4 * g4 + 3] * p.scale);
          *reinterpret_cast<uint2*>(ob + d) = pk;
        }
      }
  }
}

// ------------------------------------------------------------------------------------------ backward: dK, dV
// The workgroup (bx, h, b) of the pass: bx = key block, or with QSPLIT (query chunk, key block) with the key block fastest.  The
// single-problem kernel takes the three from its grid, the grouped one (attn_bwd_dkv_group_kernel) from its problem table.
template <int DPP, int NS, int NB, bool QSPLIT>
__device__ __forceinline__ void attn_bwd_dkv_body(const AttnParams& p, const int bx, const int h, const int b, unsigned char* smem) {
  using I = Img<DPP>;
  constexpr int STAGE = 2 * I::BYTES + 2 * KT * 4;  // Q image | dO image | lse[KT] | delta[KT]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 31, fh = lane >> 5;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int kblk = QSPLIT ? bx % p.kblocks : bx;
  const int k0 = kblk * 128;
  const int ki = k0 + wave * 32 + fr;  // this lane's key
  const float kwt = p.key_w ? p.key_w[min(ki, p.Nk - 1)] : 1.f;
  const bf16_t* qb = p.q + (long)b * p.bsq + h * p.D;
  const bf16_t* dob = p.dout + (long)b * p.bsdo + h * p.D;
  const bf16_t* kb = p.k + (long)b * p.bsk + h * p.D;
  const bf16_t* vb = p.v + (long)b * p.bsv + h * p.D;
  const float* lse_g = p.lse + ((long)b * p.H + h) * p.Nq;
  const float* dlt_g = p.delta + ((long)b * p.H + h) * p.Nq;

  TileDma<DPP> dma, dmad;
  dma.init(wave, lane, p.D);
  dmad.init(wave, lane, p.D);
  TrLane<DPP> tr;
  tr.init(lane);
  int qstart = 0, qend = p.Nq;
  if (p.causal) qstart = (k0 / KT) * KT;  // queries before the block's first key see none of its keys
  if (QSPLIT) {
    qstart = (bx / p.kblocks) * p.qchunk;
    qend = min(p.Nq, qstart + p.qchunk);
  }
  dma.bind(qb, p.ldq, qstart);
  dmad.bind(dob, p.lddo, qstart);
  auto stage = [&](int qbase, unsigned char* st) {  // (called for qstart, qstart + KT, ... in order)
    dma.issue(qbase, p.Nq, st, wave_u);
    dmad.issue(qbase, p.Nq, st + I::BYTES, wave_u);
    // per-query softmax statistics: one 4-byte DMA per lane (wave 0: lse, wave 1: delta); rows past Nq read row Nq-1 (masked)
    if (wave_u < 2) {
      const int q = min(qbase + lane, p.Nq - 1);
      glds4((wave_u == 0 ? lse_g : dlt_g) + q, st + 2 * I::BYTES + wave_u * (KT * 4));
    }
  };
  if (qstart < qend) stage(qstart, smem);

  bf16x8_t kf[NS], vf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    uint4 v = make_uint4(0, 0, 0, 0), w = make_uint4(0, 0, 0, 0);
    const int d0 = 16 * s + 8 * fh;
    if (ki < p.Nk && d0 < p.D) {
      v = *reinterpret_cast<const uint4*>(kb + (long)ki * p.ldk + d0);
      w = *reinterpret_cast<const uint4*>(vb + (long)ki * p.ldv + d0);
    }
    kf[s] = __builtin_bit_cast(bf16x8_t, v);
    vf[s] = __builtin_bit_cast(bf16x8_t, w);
  }
  f32x16_t dk_acc[NB], dv_acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) { dk_acc[i][e] = 0.f; dv_acc[i][e] = 0.f; }

  int cur = 0;
  // The tile body exists with and without the boundary / causal mask (and the key weights), and the wave-uniform choice is made
  // outside the tile loop (attn_tile_loops): a test inside the per-element loop cuts the unrolled body into 32 three-instruction
  // basic blocks (fma - exp - mul with a branch each), which nothing can be scheduled across (every exp latency exposed, no MFMA
  // beside the VALU work).
  auto tiles = [&](auto masked, auto weighted, int qfrom, int qto) {
    constexpr bool MASK = decltype(masked)::value, KW = decltype(weighted)::value;
    for (int qbase = qfrom; qbase < qto; qbase += KT, cur ^= 1) {
      dma_join();
      if (qbase + KT < qend) stage(qbase + KT, smem + (cur ^ 1) * STAGE);
      const unsigned char* q_img = smem + cur * STAGE;
      const unsigned char* do_img = q_img + I::BYTES;
      const float* lse_s = reinterpret_cast<const float*>(q_img + 2 * I::BYTES);
      const float* dlt_s = lse_s + KT;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        f32x16_t sa, dpa;
        float lrow[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          // accumulator rows 8*g4 + 4*fh + 0..3 are four consecutive queries: one 16-byte read each of lse / delta;
          // -delta seeds the dP accumulator so that dP - delta comes out of the MFMA chain
          const float4 l4 = *reinterpret_cast<const float4*>(lse_s + qt * 32 + 8 * g4 + 4 * fh);
          const float4 d4 = *reinterpret_cast<const float4*>(dlt_s + qt * 32 + 8 * g4 + 4 * fh);
          lrow[4 * g4] = l4.x; lrow[4 * g4 + 1] = l4.y; lrow[4 * g4 + 2] = l4.z; lrow[4 * g4 + 3] = l4.w;
          dpa[4 * g4] = -d4.x; dpa[4 * g4 + 1] = -d4.y; dpa[4 * g4 + 2] = -d4.z; dpa[4 * g4 + 3] = -d4.w;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) sa[e] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const bf16x8_t qf = row_frag<DPP>(q_img, qt * 32 + fr, 2 * s + fh);
          sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kf[s], sa, 0, 0, 0);
          const bf16x8_t df = row_frag<DPP>(do_img, qt * 32 + fr, 2 * s + fh);
          dpa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, vf[s], dpa, 0, 0, 0);
        }
        float pr[16], ds[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float pv = __builtin_amdgcn_exp2f(fmaf(sa[e], p.scale2, -lrow[e]));
          if (KW) pv *= kwt;
          if (MASK) {
            const int q = qbase + qt * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
            pv = (q >= p.Nq || ki >= p.Nk || (p.causal && ki > q)) ? 0.f : pv;
          }
          pr[e] = pv;
          ds[e] = pv * dpa[e];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8_t pf = cvt_frag(pr + 8 * s);
          const bf16x8_t dsf = cvt_frag(ds + 8 * s);
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const bf16x8_t dotf = tr.frag(do_img, qt * 32 + 16 * s, i);
            dv_acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotf, pf, dv_acc[i], 0, 0, 0);
            const bf16x8_t qtf = tr.frag(q_img, qt * 32 + 16 * s, i);
            dk_acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, dsf, dk_acc[i], 0, 0, 0);
          }
        }
      }
    }
  };
  attn_tile_loops(tiles, p.key_w != nullptr, p.causal || k0 + 128 > p.Nk, qstart, qend, p.Nq);
  if (QSPLIT) {  // this query chunk's partial sums go to its OWN fp32 slab (plain stores, one writer per element: no atomics, no
    // zero fill); attn_kv_finish_kernel adds the slabs in chunk order
    if (ki < p.Nk) {
      const long C = (long)p.H * p.D;
      const long slab = 2 * (long)p.B * p.Nk * C;
      float* wk = p.kv_ws + (bx / p.kblocks) * slab + ((long)b * p.Nk + ki) * C + h * p.D;
      float* wv = wk + (long)p.B * p.Nk * C;
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int d = i * 32 + 8 * g4 + 4 * fh;
          if (d < p.D) {
            *reinterpret_cast<float4*>(wk + d) = make_float4(dk_acc[i][4 * g4] * p.scale, dk_acc[i][4 * g4 + 1] * p.scale,
                                                             dk_acc[i][4 * g4 + 2] * p.scale, dk_acc[i][4 * g4 + 3] * p.scale);
            *reinterpret_cast<float4*>(wv + d) = make_float4(dv_acc[i][4 * g4], dv_acc[i][4 * g4 + 1], dv_acc[i][4 * g4 + 2], dv_acc[i][4 * g4 + 3]);
          }
        }
    }
    return;
  }
  if (ki < p.Nk) {
    bf16_t* dkb = p.dk + (long)b * p.bsdk + (long)ki * p.lddk + h * p.D;
    bf16_t* dvb = p.dv + (long)b * p.bsdv + (long)ki * p.lddv + h * p.D;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = i * 32 + 8 * g4 + 4 * fh;
        if (d < p.D) {
          uint2 pk;
          pk.x = pack2bf(dk_acc[i][4 * g4] * p.scale, dk_acc[i][4 * g4 + 1] * p.scale);
          pk.y = pack2bf(dk_acc[i][4 * g4 + 2] * p.scale, dk_acc[i][4 * g4 + 3] * p.scale);
          *reinterpret_cast<uint2*>(dkb + d) = pk;
          pk.x = pack2bf(dv_acc[i][4 * g4], dv_acc[i][4 * g4 + 1]);
          pk.y = pack2bf(dv_acc[i][4 * g4 + 2], dv_acc[i][4 * g4 + 3]);
          *reinterpret_cast<uint2*>(dvb + d) = pk;
        }
      }
  }
}

template <int DPP, int NS, int NB, bool QSPLIT>
__global__ void __launch_bounds__(256) attn_bwd_dkv_kernel(const AttnParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  attn_bwd_dkv_body<DPP, NS, NB, QSPLIT>(p, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, smem);
}

// Several dK/dV problems of one instantiation as ONE launch (sdt_attention_bwd_dkv_group): nothing on the input-gradient chain reads
// a cross-attention's dK/dV, and one alone is 32 - 256 workgroups.  Workgroups in order (problem, image, head, bx): wg_end is the
// prefix table, gx[i] the problem's extent in bx.  Every problem keeps its own plan (kv_ws set: query split into its own slabs) and
// runs the body of the single launch, so its results are those of the single launch bit for bit.
#define ATTN_GROUP_MAX 8  // problems per launch (kernel-argument space)
#define ATTN_DKV_GROUP_ABI_MAX 32  // problems per sdt_attention_bwd_dkv_group call
struct AttnGroupParams {
  int n;
  int wg_end[ATTN_GROUP_MAX];
  int gx[ATTN_GROUP_MAX];  // dK/dV: workgroups per (image, head); finishing pass: the problem's slab count
  AttnParams prob[ATTN_GROUP_MAX];
};
static_assert(sizeof(AttnGroupParams) <= 4096, "the grouped attention launches pass their problem table as kernel arguments");

__device__ __forceinline__ int attn_group_find(const AttnGroupParams& gp, int* local) {
  const int blk = blockIdx.x;
  int i = 0;
  while (i + 1 < gp.n && blk >= gp.wg_end[i]) ++i;  // wave-uniform scalar walk over <= 8 entries
  *local = blk - (i ? gp.wg_end[i - 1] : 0);
  return i;
}

template <int DPP, int NS, int NB>
__global__ void __launch_bounds__(256) attn_bwd_dkv_group_kernel(const AttnGroupParams gp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int local;
  const int i = attn_group_find(gp, &local);
  const AttnParams p = gp.prob[i];  // by value: fetched once, into scalar registers
  const int gx = gp.gx[i];
  const int rest = local / gx, bx = local - rest * gx;
  const int b = rest / p.H, h = rest - b * p.H;
  if (p.kv_ws) attn_bwd_dkv_body<DPP, NS, NB, true>(p, bx, h, b, smem);
  else attn_bwd_dkv_body<DPP, NS, NB, false>(p, bx, h, b, smem);
}

// fp32 slabs [nsplit][2][B][Nk][C] (one per query chunk) -> bf16 dk / dv (row strides lddk / lddv), 8 columns per thread; the
// slabs are added in chunk order: bitwise reproducible.  Workgroup `bid` of `nblocks`.
__device__ __forceinline__ void attn_kv_finish_body(const AttnParams& p, const int nsplit, const int bid, const int nblocks) {
  const int C = p.H * p.D, cv = C >> 3;
  const long rows = (long)p.B * p.Nk, total = rows * cv;
  const long slab = 2 * rows * C;
  for (long i = (long)bid * blockDim.x + threadIdx.x; i < total; i += (long)nblocks * blockDim.x) {
    const long r = i / cv;
    const int c = (int)(i - r * cv) * 8;
    const int b = (int)(r / p.Nk), ki = (int)(r - (long)b * p.Nk);
    float fk[8], fv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { fk[e] = 0.f; fv[e] = 0.f; }
    for (int sp = 0; sp < nsplit; ++sp) {
      const float* wk = p.kv_ws + sp * slab + r * C + c;
      const float* wv = wk + rows * C;
      const float4 a0 = *reinterpret_cast<const float4*>(wk), a1 = *reinterpret_cast<const float4*>(wk + 4);
      const float4 b0 = *reinterpret_cast<const float4*>(wv), b1 = *reinterpret_cast<const float4*>(wv + 4);
      fk[0] += a0.x; fk[1] += a0.y; fk[2] += a0.z; fk[3] += a0.w; fk[4] += a1.x; fk[5] += a1.y; fk[6] += a1.z; fk[7] += a1.w;
      fv[0] += b0.x; fv[1] += b0.y; fv[2] += b0.z; fv[3] += b0.w; fv[4] += b1.x; fv[5] += b1.y; fv[6] += b1.z; fv[7] += b1.w;
    }
    *reinterpret_cast<uint4*>(p.dk + (long)b * p.bsdk + (long)ki * p.lddk + c) = pack8(fk);
    *reinterpret_cast<uint4*>(p.dv + (long)b * p.bsdv + (long)ki * p.lddv + c) = pack8(fv);
  }
}
__global__ void __launch_bounds__(256) attn_kv_finish_kernel(const AttnParams p, int nsplit) {
  attn_kv_finish_body(p, nsplit, (int)blockIdx.x, (int)gridDim.x);
}
// the finishing passes of several split problems as one launch: each problem keeps the workgroups of its own launch
__global__ void __launch_bounds__(256) attn_kv_finish_group_kernel(const AttnGroupParams gp) {
  int local;
  const int i = attn_group_find(gp, &local);
  const AttnParams p = gp.prob[i];
  attn_kv_finish_body(p, gp.gx[i], local, gp.wg_end[i] - (i ? gp.wg_end[i - 1] : 0));
}

// query split of the dK/dV pass: used when the key blocks alone leave most of the chip idle
static int attn_qsplits(int B, int H, int Nq, int Nk, int causal) {
  if (causal) return 1;
  const long base = (long)sdt_ceil_div(Nk, 128) * H * B;
  if (base >= 128 || Nq < 1024) return 1;
  int s = (int)((256 + base - 1) / base);
  const int max_s = Nq / 256;
  if (s > max_s) s = max_s;
  return s < 2 ? 1 : s;
}
// the split plan of a problem whose slabs are at p->kv_ws: key blocks, queries per chunk; returns the number of chunks (= slabs)
static int attn_split_plan(AttnParams* p) {
  const int splits = attn_qsplits(p->B, p->H, p->Nq, p->Nk, p->causal);
  p->kblocks = sdt_ceil_div(p->Nk, 128);
  p->qchunk = sdt_ceil_div(sdt_ceil_div(p->Nq, splits), KT) * KT;
  return sdt_ceil_div(p->Nq, p->qchunk);
}
static int attn_finish_blocks(const AttnParams& p) { return sdt_grid_1d((long)p.B * p.Nk * p.H * p.D / 8, 256, 1024); }

// ================================================================== C ABI
static int attn_fill(AttnParams* p, const SdtAttnDesc* d, const char* name) {
  SDT_CHECK_ARG(d, "%s: null descriptor", name);
  SDT_CHECK_ARG(d->B > 0 && d->H > 0 && d->Nq > 0 && d->Nk > 0 && d->D > 0 && d->B <= 65535 && d->H <= 65535,
                "%s: bad shape B=%d H=%d Nq=%d Nk=%d D=%d", name, d->B, d->H, d->Nq, d->Nk, d->D);
  SDT_CHECK_ARG(d->D % 8 == 0 && d->D <= 160, "%s: head dim %d must be a multiple of 8 and <= 160", name, d->D);
  SDT_CHECK_ARG(d->ldq % 8 == 0 && d->ldk % 8 == 0 && d->ldv % 8 == 0 && d->ldo % 8 == 0, "%s: row strides must be multiples of 8", name);
  SDT_CHECK_ARG(d->ldq < (1 << 24) && d->ldk < (1 << 24) && d->ldv < (1 << 24) && d->ldo < (1 << 24) && d->ld_dout < (1 << 24),
                "%s: row strides must be below 2^24 elements (a tile's byte step is kept in 32 bits)", name);
  p->B = d->B; p->H = d->H; p->Nq = d->Nq; p->Nk = d->Nk; p->D = d->D;
  p->ldq = d->ldq; p->ldk = d->ldk; p->ldv = d->ldv; p->ldo = d->ldo;
  p->bsq = (long)d->Nq * d->ldq; p->bsk = (long)d->Nk * d->ldk; p->bsv = (long)d->Nk * d->ldv; p->bso = (long)d->Nq * d->ldo;
  p->lddo = d->ldo; p->bsdo = p->bso;
  p->lddq = d->ldq; p->bsdq = p->bsq; p->lddk = d->ldk; p->bsdk = p->bsk; p->lddv = d->ldv; p->bsdv = p->bsv;
  p->scale = d->scale;
  p->scale2 = d->scale * 1.4426950408889634f;
  p->causal = d->causal;
  p->key_w = d->key_weight;
  return SDT_OK;
}

template <typename K>
static void ensure_lds(K kernel, size_t lds, bool* done) {  // once per instantiation (also keeps it out of graph captures)
  if (!*done) {
    hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    *done = true;
  }
}
template <int DPP, int NS, int NB>
static void launch_fwd(const AttnParams& p, hipStream_t stream) {
  static_assert(NB * 32 <= DPP && NS * 16 <= DPP, "image pitch too small");
  static bool set_m = false, set_a = false;
  const size_t lds = (size_t)2 * 2 * Img<DPP>::BYTES;
  const dim3 grid(sdt_ceil_div(p.Nq, 128), p.H, p.B);
  if (p.D <= NB * 32 - 8) {  // a spare padded feature carries the ones column
    ensure_lds(attn_fwd_kernel<DPP, NS, NB, true>, lds, &set_m);
    hipLaunchKernelGGL((attn_fwd_kernel<DPP, NS, NB, true>), grid, dim3(256), lds, stream, p);
  } else {
    ensure_lds(attn_fwd_kernel<DPP, NS, NB, false>, lds, &set_a);
    hipLaunchKernelGGL((attn_fwd_kernel<DPP, NS, NB, false>), grid, dim3(256), lds, stream, p);
  }
}
template <int DPP, int NS, int NB>
static void launch_bwd(const AttnParams& p, bool with_dkv, hipStream_t stream) {  // with_dkv false: the dQ pass (and delta) alone
  static_assert(NB * 32 <= DPP && NS * 16 <= DPP, "image pitch too small");
  static bool set_q = false, set_kv = false;
  const size_t lds_dq = (size_t)2 * 2 * Img<DPP>::BYTES;
  const size_t lds_dkv = (size_t)2 * (2 * Img<DPP>::BYTES + 2 * KT * sizeof(float));
  static bool set_kvs = false;
  ensure_lds(attn_bwd_dq_kernel<DPP, NS, NB>, lds_dq, &set_q);
  hipLaunchKernelGGL((attn_bwd_dq_kernel<DPP, NS, NB>), dim3(sdt_ceil_div(p.Nq, 128), p.H, p.B), dim3(256), lds_dq, stream, p);
  if (!with_dkv) return;
  if (p.kv_ws) {
    AttnParams ps = p;
    const int nsplit = attn_split_plan(&ps);
    ensure_lds(attn_bwd_dkv_kernel<DPP, NS, NB, true>, lds_dkv, &set_kvs);
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<DPP, NS, NB, true>), dim3(ps.kblocks * nsplit, p.H, p.B), dim3(256), lds_dkv, stream, ps);
    hipLaunchKernelGGL(attn_kv_finish_kernel, dim3(attn_finish_blocks(p)), dim3(256), 0, stream, ps, nsplit);
  } else {
    ensure_lds(attn_bwd_dkv_kernel<DPP, NS, NB, false>, lds_dkv, &set_kv);
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<DPP, NS, NB, false>), dim3(sdt_ceil_div(p.Nk, 128), p.H, p.B), dim3(256), lds_dkv, stream, p);
  }
}
template <int DPP, int NS, int NB>
static void launch_dkv_group(const AttnGroupParams& gp, hipStream_t stream) {
  static bool set_g = false;
  const size_t lds_dkv = (size_t)2 * (2 * Img<DPP>::BYTES + 2 * KT * sizeof(float));
  ensure_lds(attn_bwd_dkv_group_kernel<DPP, NS, NB>, lds_dkv, &set_g);
  hipLaunchKernelGGL((attn_bwd_dkv_group_kernel<DPP, NS, NB>), dim3(gp.wg_end[gp.n - 1]), dim3(256), lds_dkv, stream, gp);
}

// the kernel instantiation <DPP, NS, NB> of a head dim, as an index (attn_bwd_dispatch / attn_dkv_group_dispatch)
static int attn_class(int D) { return D <= 48 ? 0 : D <= 64 ? 1 : D <= 80 ? 2 : D <= 96 ? 3 : D <= 128 ? 4 : 5; }
static void attn_bwd_dispatch(const AttnParams& p, bool with_dkv, hipStream_t stream) {
  switch (attn_class(p.D)) {
    case 0: launch_bwd<64, 3, 2>(p, with_dkv, stream); break;
    case 1: launch_bwd<64, 4, 2>(p, with_dkv, stream); break;
    case 2: launch_bwd<128, 5, 3>(p, with_dkv, stream); break;
    case 3: launch_bwd<128, 6, 3>(p, with_dkv, stream); break;
    case 4: launch_bwd<128, 8, 4>(p, with_dkv, stream); break;
    default: launch_bwd<256, 10, 5>(p, with_dkv, stream); break;
  }
}
static void attn_dkv_group_dispatch(int cls, const AttnGroupParams& gp, hipStream_t stream) {
  switch (cls) {
    case 0: launch_dkv_group<64, 3, 2>(gp, stream); break;
    case 1: launch_dkv_group<64, 4, 2>(gp, stream); break;
    case 2: launch_dkv_group<128, 5, 3>(gp, stream); break;
    case 3: launch_dkv_group<128, 6, 3>(gp, stream); break;
    case 4: launch_dkv_group<128, 8, 4>(gp, stream); break;
    default: launch_dkv_group<256, 10, 5>(gp, stream); break;
  }
}
// descriptor + operand pointers -> the kernels' parameters (the backward's strides included); kv_ws is left to the caller
static int attn_fill_bwd(AttnParams* p, const SdtAttnDesc* desc, const char* name, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                         const uint16_t* out, const uint16_t* dout, const float* lse, const float* delta, uint16_t* dq, uint16_t* dk,
                         uint16_t* dv) {
  int rc = attn_fill(p, desc, name);
  if (rc) return rc;
  p->q = (const bf16_t*)q; p->k = (const bf16_t*)k; p->v = (const bf16_t*)v; p->o = (const bf16_t*)out;
  p->dout = (const bf16_t*)dout; p->lse = const_cast<float*>(lse); p->delta = delta;
  p->dq = (bf16_t*)dq; p->dk = (bf16_t*)dk; p->dv = (bf16_t*)dv;
  if (desc->ldgrad_q) { p->lddq = desc->ldgrad_q; p->bsdq = (long)p->Nq * p->lddq; }
  if (desc->ldgrad_k) { p->lddk = desc->ldgrad_k; p->bsdk = (long)p->Nk * p->lddk; }
  if (desc->ldgrad_v) { p->lddv = desc->ldgrad_v; p->bsdv = (long)p->Nk * p->lddv; }
  if (desc->ld_dout) { p->lddo = desc->ld_dout; p->bsdo = (long)p->Nq * p->lddo; }
  return SDT_OK;
}

extern "C" {

int sdt_attention_fwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, float* lse,
                      const SdtAttnDesc* desc, hipStream_t stream) {
  SDT_CHECK_ARG(q && k && v && out, "sdt_attention_fwd: null pointer");
  AttnParams p = {};
  int rc = attn_fill(&p, desc, "sdt_attention_fwd");
  if (rc) return rc;
  SDT_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0, "sdt_attention_fwd: pointers must be 16-byte aligned");
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.out = (bf16_t*)out; p.lse = lse;
  const int D = p.D;
  if (D <= 48) launch_fwd<64, 3, 2>(p, stream);
  else if (D <= 64) launch_fwd<64, 4, 2>(p, stream);
  else if (D <= 80) launch_fwd<128, 5, 3>(p, stream);
  else if (D <= 96) launch_fwd<128, 6, 3>(p, stream);
  else if (D <= 128) launch_fwd<128, 8, 4>(p, stream);
  else launch_fwd<256, 10, 5>(p, stream);
  SDT_LAUNCH_CHECK("sdt_attention_fwd");
  return SDT_OK;
}

/* scratch for sdt_attention_bwd: B*H*Nq floats (delta) + one 2*B*Nk*H*D-float slab per query chunk when the dK/dV pass splits the
 * query range (each chunk writes its own slab, a finishing pass adds them in order: no atomics) */
int64_t sdt_attention_bwd_workspace_bytes(const SdtAttnDesc* d) {
  if (!d || d->B <= 0 || d->H <= 0 || d->Nq <= 0 || d->Nk <= 0 || d->D <= 0) return 0;
  return sdt_attention_bwd_delta_bytes(d) + sdt_attention_bwd_slab_bytes(d);
}
/* the two parts of that scratch: delta (rounded up to 16 bytes), and the slabs of the split dK/dV pass (0 when it does not split) */
int64_t sdt_attention_bwd_delta_bytes(const SdtAttnDesc* d) {
  if (!d || d->B <= 0 || d->H <= 0 || d->Nq <= 0 || d->Nk <= 0 || d->D <= 0) return 0;
  return ((int64_t)d->B * d->H * d->Nq + 3) / 4 * 4 * (int64_t)sizeof(float);
}
int64_t sdt_attention_bwd_slab_bytes(const SdtAttnDesc* d) {
  if (!d || d->B <= 0 || d->H <= 0 || d->Nq <= 0 || d->Nk <= 0 || d->D <= 0) return 0;
  const int qs = attn_qsplits(d->B, d->H, d->Nq, d->Nk, d->causal);
  return qs > 1 ? (int64_t)qs * 2 * d->B * d->Nk * d->H * d->D * (int64_t)sizeof(float) : 0;
}

// workspace: sdt_attention_bwd_workspace_bytes(desc) bytes (at least B*H*Nq floats: without the rest the query split is not used)
int sdt_attention_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* out, const uint16_t* dout,
                      const float* lse, uint16_t* dq, uint16_t* dk, uint16_t* dv, float* delta_ws, int64_t workspace_bytes,
                      const SdtAttnDesc* desc, hipStream_t stream) {
  SDT_CHECK_ARG(q && k && v && out && dout && lse && dq && dk && dv && delta_ws, "sdt_attention_bwd: null pointer");
  SDT_CHECK_ARG(desc && workspace_bytes >= (int64_t)sizeof(float) * desc->B * desc->H * desc->Nq, "sdt_attention_bwd: workspace too small");
  AttnParams p = {};
  int rc = attn_fill_bwd(&p, desc, "sdt_attention_bwd", q, k, v, out, dout, lse, delta_ws, dq, dk, dv);
  if (rc) return rc;
  if (attn_qsplits(p.B, p.H, p.Nq, p.Nk, p.causal) > 1 && workspace_bytes >= sdt_attention_bwd_workspace_bytes(desc))
    p.kv_ws = delta_ws + ((long)p.B * p.H * p.Nq + 3) / 4 * 4;
  attn_bwd_dispatch(p, true, stream);
  SDT_LAUNCH_CHECK("sdt_attention_bwd");
  return SDT_OK;
}

// the dQ pass of sdt_attention_bwd alone: dq, and delta (B*H*Nq floats) for a later sdt_attention_bwd_dkv_group
int sdt_attention_bwd_dq(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* out, const uint16_t* dout,
                         const float* lse, uint16_t* dq, float* delta, const SdtAttnDesc* desc, hipStream_t stream) {
  SDT_CHECK_ARG(q && k && v && out && dout && lse && dq && delta && desc, "sdt_attention_bwd_dq: null pointer");
  AttnParams p = {};
  int rc = attn_fill_bwd(&p, desc, "sdt_attention_bwd_dq", q, k, v, out, dout, lse, delta, dq, nullptr, nullptr);
  if (rc) return rc;
  attn_bwd_dispatch(p, false, stream);
  SDT_LAUNCH_CHECK("sdt_attention_bwd_dq");
  return SDT_OK;
}

int sdt_attention_bwd_dkv_group_max(void) { return ATTN_DKV_GROUP_ABI_MAX; }

int sdt_attention_bwd_dkv_group(const SdtAttnDkvProblem* problems, int n, hipStream_t stream) {
  SDT_CHECK_ARG(problems && n > 0 && n <= ATTN_DKV_GROUP_ABI_MAX, "sdt_attention_bwd_dkv_group: 1..%d problems", ATTN_DKV_GROUP_ABI_MAX);
  static thread_local AttnParams ps[ATTN_DKV_GROUP_ABI_MAX];
  static thread_local int nsplit[ATTN_DKV_GROUP_ABI_MAX], gxs[ATTN_DKV_GROUP_ABI_MAX];
  long all_wgs = 0;  // every check runs before the first launch: a refused table launches nothing
  for (int i = 0; i < n; ++i) {
    const SdtAttnDkvProblem& q = problems[i];
    SDT_CHECK_ARG(q.q && q.k && q.v && q.dout && q.lse && q.delta && q.dk && q.dv, "sdt_attention_bwd_dkv_group: problem %d: null pointer", i);
    SDT_CHECK_ARG((((uintptr_t)q.q | (uintptr_t)q.k | (uintptr_t)q.v | (uintptr_t)q.dout | (uintptr_t)q.dk | (uintptr_t)q.dv |
                    (uintptr_t)q.slabs | (uintptr_t)q.lse | (uintptr_t)q.delta) & 15) == 0,
                  "sdt_attention_bwd_dkv_group: problem %d: pointers must be 16-byte aligned", i);
    ps[i] = AttnParams{};
    int rc = attn_fill_bwd(&ps[i], &q.desc, "sdt_attention_bwd_dkv_group", q.q, q.k, q.v, nullptr, q.dout, q.lse, q.delta, nullptr, q.dk, q.dv);
    if (rc) return rc;
    SDT_CHECK_ARG(ps[i].lddk % 8 == 0 && ps[i].lddv % 8 == 0 && ps[i].lddo % 8 == 0,
                  "sdt_attention_bwd_dkv_group: problem %d: row strides must be multiples of 8", i);
    nsplit[i] = 0;  // the plan of the single call with its full workspace: split where attn_qsplits says so, into the problem's own slabs
    if (attn_qsplits(ps[i].B, ps[i].H, ps[i].Nq, ps[i].Nk, ps[i].causal) > 1) {
      SDT_CHECK_ARG(q.slabs, "sdt_attention_bwd_dkv_group: problem %d: slabs of sdt_attention_bwd_slab_bytes() needed", i);
      ps[i].kv_ws = q.slabs;
      nsplit[i] = attn_split_plan(&ps[i]);
    }
    gxs[i] = nsplit[i] ? ps[i].kblocks * nsplit[i] : sdt_ceil_div(ps[i].Nk, 128);
    all_wgs += (long)gxs[i] * ps[i].H * ps[i].B;  // (an upper bound of any one launch's grid)
    SDT_CHECK_ARG(all_wgs < (1L << 30), "sdt_attention_bwd_dkv_group: too many workgroups");
  }
  AttnGroupParams gp;
  for (int cls = 0; cls < 6; ++cls) {  // one launch per kernel instantiation present (ATTN_GROUP_MAX problems per launch)
    gp.n = 0;
    for (int i = 0; i <= n; ++i) {
      if (i < n && attn_class(ps[i].D) == cls) {
        const AttnParams& p = ps[i];
        gp.prob[gp.n] = p;
        gp.gx[gp.n] = gxs[i];
        gp.wg_end[gp.n] = gxs[i] * p.H * p.B + (gp.n ? gp.wg_end[gp.n - 1] : 0);
        ++gp.n;
      }
      if (gp.n == ATTN_GROUP_MAX || (i == n && gp.n > 0)) {
        attn_dkv_group_dispatch(cls, gp, stream);
        gp.n = 0;
      }
    }
  }
  gp.n = 0;
  for (int i = 0; i <= n; ++i) {  // the finishing passes of all split problems
    if (i < n && nsplit[i]) {
      gp.prob[gp.n] = ps[i];
      gp.gx[gp.n] = nsplit[i];
      gp.wg_end[gp.n] = attn_finish_blocks(ps[i]) + (gp.n ? gp.wg_end[gp.n - 1] : 0);
      ++gp.n;
    }
    if (gp.n == ATTN_GROUP_MAX || (i == n && gp.n > 0)) {
      hipLaunchKernelGGL(attn_kv_finish_group_kernel, dim3(gp.wg_end[gp.n - 1]), dim3(256), 0, stream, gp);
      gp.n = 0;
    }
  }
  SDT_LAUNCH_CHECK("sdt_attention_bwd_dkv_group");
  return SDT_OK;
}

}  // extern "C"
