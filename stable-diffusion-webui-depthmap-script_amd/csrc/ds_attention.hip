// ds_attention_fwd: fused (flash-style) attention forward for the ViT encoders of the depth models, on the gfx950
// matrix cores.  Replaces, per transformer block, the reference's
//     attn = (q * scale) @ k^T [+ relative_position_bias];  attn = softmax(attn);  x = attn @ v
// (ddepth_anything_v2/depth_anything_v2/dinov2_layers/attention.py:49-62, dmidas/backbones/beit.py:65-91), which
// materialises a B x H x N x N tensor in HBM, by one kernel that never leaves the chip between Q.K^T and P.V.
//
// Operands (head_dim is 64 for every encoder the reference ships):
//   qk   [B, Np, 2, H, 64]  f16/bf16   Q and K exactly as the projection GEMM writes them (token major)
//   vt   [B, H*64, Np]      f16/bf16   V TRANSPOSED (key index contiguous), produced in that layout by its own GEMM
//   bias optional: the operand made by ds_attention_bias_pack (this file) from the [H, n, n] table -- in units of 1/scale,
//        zero padded to whole 64-key tiles, stored as the A fragments of the MFMAs that add it to the logits
//   out  [B, Np, H*64]      f16/bf16
// Np (the token stride) is a multiple of 8; keys >= n_valid are masked (pad rows of the padded token sequence).
//
// Mapping: workgroup = 4 waves of one (batch, head); a wave owns NQB = 1 or 2 blocks of 32 query rows (128 or 256 rows per
// workgroup).  Per 64-key tile and 32-query block:
//   S^T = Bias^T . I + K . Q^T   "swapped" so that a lane holds logits of ONE query (column lane&31) for 32 of the 64 keys:
//                   the row max / row sum of the online softmax are in-lane reductions plus one exchange with lane^32;
//                   2 key blocks x (2 bias + 4 d-slices) of v_mfma_f32_32x32x16 (A = K rows from LDS, B = Q rows in registers)
//   O^T += V^T . P^T  A = V^T rows (one ds_read_b128 per fragment), B = P^T built in registers straight from the S^T
//                   accumulators: the accumulator's row order fixes which keys sit in which k-slot, and V^T is stored in
//                   LDS in that key order, so no cross-lane traffic is needed between the two GEMMs.
// K and V^T tiles sit in LDS in padded 144-byte rows (conflict-free ds_read_b128).  The next tile is fetched into registers
// (buffer loads through descriptors) while the current one is computed and stashed into the other of two LDS buffers: one
// barrier per tile.  Workgroups are ordered so that one XCD's L2 serves all query blocks of a (batch, head) and one head's
// bias (see the kernel).
//
// This is the second generation of the kernel and the only one in this file.  Generation 1 (32 rows per wave, bias added on the
// vector pipe), generation 3 (generation 2 skewed by one tile inside the wave), the timing-ablation masks and the phase clock
// were removed: their measurements are in DESIGN.md 3.6, DESIGN_HISTORY.md and profiles/, their code in git history.
// Generation 4 (ds_attention4.hip) is selected only by DS_ATT_GEN=4.
#include "ds_attention.h"

// =====================================================================================================================
// k_attention_fwd2<BF16, HAS_BIAS, NQB, LATE>.
//
// (A "version 3" was built and measured in round 2 and removed again -- git history, profiles/round2_attention_v3_experiment.txt:
// one 8-wave workgroup = two independent 4-wave tasks whose wave-rows alternate, barrier by barrier, between an MFMA part
// (P.V of tile t, S of tile t+1) and a vector part (fragment reads, LDS-DMA of K / V^T three tiles ahead, softmax), the
// structure of csrc/ds_linear.hip.  Correct at the benchmark shapes, but 15-35 % SLOWER than this kernel (N = 1025 + bias:
// 0.344 vs 0.298 ms): with exactly two waves per SIMD the vector part -- ~200 instructions from ONE wave -- is bound by
// that wave's issue rate, and the softmax of a 64-wide head is as long as its MFMAs; the GEMM's memory part is 16
// instructions.  What remains is instruction-level interleaving inside a wave, i.e. a hand-scheduled kernel.)
//
// What shapes it (round-1 profile of generation 1: MFMA busy 20-26 %, ~200 VALU instructions per 16 MFMA with the bias):
//   * NQB = 32-row query blocks per wave.  2: 64 rows per wave, 256 per workgroup -- every K / V^T fragment read from LDS feeds
//     TWO MFMAs, and K / V^T / the staging traffic per query row halve; two fat waves per SIMD (<= 256 VGPRs).  1: 32 rows per
//     wave, three waves per SIMD, four with LATE.  ds_attention_fwd chooses by sequence length.
//   * the relative-position bias enters through the MATRIX pipe:  S^T = K.Q^T + Bias^T.I  with a constant identity B operand
//     (2 extra MFMAs per 32 x 32 logits block, exact: an f16 value times 1.0 accumulated in float32).  The packed operand is
//     stored as MFMA A fragments, in units of 1/scale (x8: exact), so the logits need NO per-element VALU work before the
//     softmax: 64 v_fma_mix + unpacking per tile become 8 MFMAs on a pipe that was three quarters idle.
//   * deferred running maximum: a query's maximum is only raised (and O rescaled) when it grows by more than 2^AT2_THR;
//     probabilities are then bounded by 2^AT2_THR instead of 1, harmless in f16/bf16 with float32 accumulation.
//   * K and V^T tiles use padded 144-byte rows (conflict-free ds_read_b128 for both), and V^T is stored key-permuted so that a
//     P.V fragment is ONE ds_read_b128: within every 16 keys the order is [0-3, 8-11, 4-7, 12-15] -- the k-slot order the S^T
//     accumulator hands to the P^T operand.
//   * s_setprio raises the wave's priority around the two MFMA clusters (S and P.V).
//   * LATE (NQB = 1 only): late fetches -- the bias of a tile is requested at the top of that tile, K / V^T of the next one
//     after S -- to fit 128 VGPRs: 4 waves per SIMD.  Wins without a bias, loses with one (numbers in ds_attention_fwd).
// (Round 4 measured software-pipelined fragment reads -- the K / V^T fragments of slice s + 2 requested while slice s is multiplied,
// the first four ahead of the bias MFMAs, the two key blocks' accumulators alternating -- against this loop, whose S and P.V
// phases compile to "two reads, wait, two dependent MFMAs" four times each: 0.289 vs 0.285 ms at N = 1025 + bias, 0.375 vs 0.386 at
// N = 1370, 0.250 vs 0.250 at N = 2443, 0.848 vs 0.819 at N = 4097 + bias.  Three waves per SIMD already cover those round trips;
// the variant was removed.)
template <int BF16, int HAS_BIAS, int NQB, bool LATE>
__global__ __launch_bounds__(AT_THREADS, NQB == 2 ? 2 : (LATE ? 4 : 3)) void k_attention_fwd2(AttnParams P)
{
    typedef at_traits<BF16> TR;
    typedef typename TR::T T;
    typedef typename TR::V8 V8;
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * AT2_TILE];       // K[2], V^T[2]: 36,864 B
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
    int L = blockIdx.x;
    if (P.chunk > 0) {                                          // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs (id & 7),
                                                                // XCD j takes the contiguous range [j*chunk, (j+1)*chunk) of work items
        L = (int)(blockIdx.x & 7) * P.chunk + (int)(blockIdx.x >> 3);
        if (L >= P.total) return;
    }
    // Work order inside an XCD's range.  Default: query blocks fastest -- the workgroups in flight on one L2 share the K / V^T
    // of one (batch, head), and a head's bias (2.4 MB at 1088 tokens) is read by one XCD only.  P.flags & 2: BATCH fastest
    // -- for sequences whose bias no longer fits an L2 (4160 tokens: 34.6 MB per head) the workgroups in flight then read
    // the SAME bias tiles at the same time (B of them per tile: one HBM read serves the batch), at the price of B times as
    // many K / V^T streams through that L2 (1 MB each).
    int qblk, b, h;
    if (P.flags & 2) { b = L % P.B; qblk = (L / P.B) % P.nq; h = L / (P.B * P.nq); }
    else { qblk = L % P.nq; b = (L / P.nq) % P.B; h = L / (P.nq * P.B); }
    const int q0 = qblk * (128 * NQB) + wave * (32 * NQB);
    // Np = token STRIDE of the operands (rows that exist per batch element, a multiple of 8); the key tiles and the packed
    // bias run on Np64, the stride rounded up to whole 64-key tiles.  Rows in [Np, Np64) do not exist: K rows there read as
    // zeros (the buffer descriptor ends at the batch element), V^T columns there alias the next row -- both are pad keys
    // (>= n_valid), whose probabilities are exactly 0 -- and query rows there are neither loaded nor stored.
    const int Np = P.Np, H = P.H;
    const int Np64 = (Np + 63) & ~63;
    const size_t tok_stride = (size_t)2 * H * AT_D;
    const T *qk = (const T *)P.qk + (size_t)b * Np * tok_stride;
    const T *q_base = qk + (size_t)h * AT_D;
    const T *k_base = qk + (size_t)(H + h) * AT_D;
    const T *vt = (const T *)P.vt + ((size_t)b * H + h) * AT_D * (size_t)Np;
    T *out_base = (T *)P.out + (size_t)b * Np * (size_t)(H * AT_D) + (size_t)h * AT_D;
    // a block with a handful of live rows (round 6): one GEMV per row instead of the tiled path (ds_attention.h: at_tail_rows)
    const int rows_live = P.n_valid - qblk * (128 * NQB);
    if (rows_live > 0 && rows_live <= AT_TAIL_ROWS && Np64 <= AT_TAIL_MAXN && (P.flags & 4)) {
        for (int row = qblk * (128 * NQB) + rows_live + (tid >> 3); row < min(Np, (qblk + 1) * (128 * NQB)); row += AT_THREADS / 8)
            *reinterpret_cast<uint4 *>(out_base + (size_t)row * (H * AT_D) + 8 * (tid & 7)) = make_uint4(0, 0, 0, 0);
        at_tail_rows<BF16, HAS_BIAS>(P, smem, b, h, qblk * (128 * NQB), rows_live);
        return;
    }
    // a wave whose rows are all padding only helps staging; its output rows are zeroed (they feed the next GEMM as ordinary
    // rows and must stay finite), rows >= Np do not exist
    const bool wave_live = q0 < P.n_valid;
    if (!wave_live && q0 < Np) {
        const int row = q0 + lane;
        if (row < Np && lane < 32 * NQB) {
            uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int c = 0; c < 8; c++) *reinterpret_cast<uint4 *>(out_base + (size_t)row * (H * AT_D) + 8 * c) = z;
        }
    }

    V8 qf[2][4];
#pragma unroll
    for (int qb = 0; qb < NQB; qb++) {
        const int qrow = min(q0 + 32 * qb + l31, Np - 1);
        const T *qp = q_base + (size_t)qrow * tok_stride + 8 * hi;
#pragma unroll
        for (int s = 0; s < 4; s++) qf[qb][s] = *reinterpret_cast<const V8 *>(qp + 16 * s);
    }
    // identity B operand of the bias MFMAs: element t of slice s is I[k = 16 s + 8 hi + t][column l31]
    V8 ident[2];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int t = 0; t < 8; t++) ident[s][t] = TR::from_f32((16 * s + 8 * hi + t) == l31 ? 1.0f : 0.0f);

    f32x16 o_acc[2][2];
#pragma unroll
    for (int qb = 0; qb < 2; qb++)
#pragma unroll
        for (int d = 0; d < 2; d++)
#pragma unroll
            for (int r = 0; r < 16; r++) o_acc[qb][d][r] = 0.f;
    float m_run[2] = { -__builtin_inff(), -__builtin_inff() }, l_run[2] = { 0.f, 0.f };

    const int st_row = tid >> 3, st_chunk = tid & 7;
    u32x4 kreg0, kreg1, vreg0, vreg1;
    const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc(
        (void *)k_base, 0, (int)(((size_t)Np * tok_stride - (size_t)(H + h) * AT_D) * sizeof(T)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void *)vt, 0, (int)((size_t)AT_D * Np * sizeof(T)), 0x00020000);
    const int vo_k = (int)((st_row * tok_stride + 8 * st_chunk) * sizeof(T));
    const int vo_v = (int)((st_row * Np + 8 * st_chunk) * sizeof(T));
    const int so_k32 = (int)(32 * tok_stride * sizeof(T)), so_r32 = (int)(32 * Np * sizeof(T));
#define A2_FETCH(kt_) do {                                                                                             \
        const int key0_ = (kt_) * AT_KB;                                                                                \
        const int sk_ = __builtin_amdgcn_readfirstlane(key0_ * (int)(tok_stride * sizeof(T)));                          \
        const int sv_ = __builtin_amdgcn_readfirstlane(key0_ * (int)sizeof(T));                                         \
        kreg0 = __builtin_amdgcn_raw_buffer_load_b128(rs_k, vo_k, sk_, 0);                                              \
        kreg1 = __builtin_amdgcn_raw_buffer_load_b128(rs_k, vo_k, sk_ + so_k32, 0);                                     \
        vreg0 = __builtin_amdgcn_raw_buffer_load_b128(rs_v, vo_v, sv_, 0);                                              \
        vreg1 = __builtin_amdgcn_raw_buffer_load_b128(rs_v, vo_v, sv_ + so_r32, 0);                                     \
    } while (0)
    // K row r, chunk c -> r*144 + 16c.  V^T row d, chunk c (keys 8c .. 8c+7) -> the permuted order described above: the low
    // four keys go to chunk (c & ~1), the high four to chunk (c | 1), each at byte offset 8 (c & 1)
    const int vst_lo = ((st_chunk & ~1) << 4) + ((st_chunk & 1) << 3), vst_hi = vst_lo + 16;
#define A2_STASH1(buf_, row_, kr_, vr_) do {                                                                            \
        *reinterpret_cast<u32x4 *>(smem + (buf_) * AT2_TILE + (row_) * AT2_ROW + (st_chunk << 4)) = kr_;                \
        unsigned char *vd_ = smem + (2 + (buf_)) * AT2_TILE + (row_) * AT2_ROW;                                         \
        *reinterpret_cast<uint2 *>(vd_ + vst_lo) = make_uint2(vr_.x, vr_.y);                                            \
        *reinterpret_cast<uint2 *>(vd_ + vst_hi) = make_uint2(vr_.z, vr_.w);                                            \
    } while (0)
    // Bias: [head][32-query block][64-key tile][chunk c = 2 kb + s][64 lanes][8]: lane (hi, l31) of chunk c holds
    // bias[query 16 s + 8 hi + t][key 32 kb + l31] / scale, t = 0..7 -- the A fragment of the MFMA that adds it.
    u32x4 breg[2][4];                                           // (unused, and eliminated, without a bias)
    const int n_kt = Np64 / AT_KB;
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(HAS_BIAS ? (const T *)P.bias + (size_t)h * Np64 * (size_t)Np64 : (const T *)P.qk), 0,
        (int)((size_t)Np64 * Np64 * sizeof(T)), 0x00020000);
    const int vo_b = (int)((((size_t)(q0 / 32) * n_kt) * 2048 + (size_t)lane * 8) * sizeof(T));
    const int so_bq = (int)((size_t)n_kt * 2048 * sizeof(T));                               // next 32-query block
#define A2_FETCH_BIAS(kt_) do {                                                                                        \
        const int sb_ = __builtin_amdgcn_readfirstlane((kt_) * (int)(2048 * sizeof(T)));                                \
        _Pragma("unroll") for (int qb_ = 0; qb_ < NQB; qb_++)                                                           \
        _Pragma("unroll") for (int c_i = 0; c_i < 4; c_i++)                                                             \
            breg[qb_][c_i] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, vo_b + qb_ * so_bq + c_i * 1024, sb_, 0);     \
    } while (0)

    const int ntiles = (P.n_valid + AT_KB - 1) / AT_KB;
    const float c_ = P.c_exp;                                   // scale * log2(e): the bias is stored in units of 1/scale
    const float thr_x = AT2_THR / c_;
    A2_FETCH(0);
    if (HAS_BIAS && wave_live && !LATE) A2_FETCH_BIAS(0);
    A2_STASH1(0, st_row, kreg0, vreg0);
    A2_STASH1(0, st_row + 32, kreg1, vreg1);
    __syncthreads();
    // One 64-key tile.  MASKED is a compile-time flag: only the last tile can hold pad keys, so the steady-state body has no
    // mask code and no control flow besides the (rare) rescale.
    auto tile = [&](const int kt, auto masked_tag) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const int cur = kt & 1;
        const unsigned char *s_k = smem + cur * AT2_TILE, *s_v = smem + (2 + cur) * AT2_TILE;
        const bool more = kt + 1 < ntiles;
        // next tile's K / V^T: in flight while this tile is computed.  LATE requests them after S, where the register pressure
        // has passed its peak (the softmax and P.V still cover an L2 round trip), and this tile's bias here instead
        if (more && (!LATE || !wave_live)) A2_FETCH(kt + 1);
        if (HAS_BIAS && LATE && wave_live) A2_FETCH_BIAS(kt);
        if (wave_live) {
            const int key0 = kt * AT_KB;
            f32x16 s_acc[2][2];
            V8 pf[2][2][2];
            float alpha[2];
            bool grow[2];
            // S^T = Bias^T.I (+) K.Q^T of query block qb_, key block kb_: the two bias MFMAs start the accumulation chain
#define A2_S_BIAS(qb_, kb_) do {                                                                                       \
                if (HAS_BIAS) {                                                                                         \
                    f32x16 z_;                                                                                          \
                    _Pragma("unroll") for (int r_ = 0; r_ < 16; r_++) z_[r_] = 0.f;                                     \
                    union { u32x4 u; V8 v; } b0_, b1_;                                                                  \
                    b0_.u = breg[qb_][2 * (kb_)]; b1_.u = breg[qb_][2 * (kb_) + 1];                                     \
                    s_acc[qb_][kb_] = TR::mfma(b0_.v, ident[0], z_);                                                    \
                    s_acc[qb_][kb_] = TR::mfma(b1_.v, ident[1], s_acc[qb_][kb_]);                                       \
                } else {                                                                                                \
                    _Pragma("unroll") for (int r_ = 0; r_ < 16; r_++) s_acc[qb_][kb_][r_] = 0.f;                        \
                }                                                                                                       \
            } while (0)
#define A2_MASK(qb_) do {                                                                                              \
                if (MASKED) {                                                                                           \
                    _Pragma("unroll") for (int kb_ = 0; kb_ < 2; kb_++)                                                 \
                    _Pragma("unroll") for (int r_ = 0; r_ < 16; r_++)                                                   \
                        if (key0 + kb_ * 32 + at_crow(r_, hi) >= P.n_valid) s_acc[qb_][kb_][r_] = -__builtin_inff();    \
                }                                                                                                       \
            } while (0)
            // online softmax of one 32-query block in the exp2 domain with a deferred maximum: the running maximum is only
            // raised when it would grow by more than the threshold (first tile: from -inf); alpha = 1 when kept
#define A2_SOFTMAX(qb_) do {                                                                                           \
                float mx_ = at_max3(s_acc[qb_][0][0], s_acc[qb_][1][0], s_acc[qb_][0][1]);                              \
                mx_ = at_max3(mx_, s_acc[qb_][1][1], s_acc[qb_][0][2]);                                                 \
                mx_ = at_max3(mx_, s_acc[qb_][1][2], s_acc[qb_][0][3]);                                                 \
                _Pragma("unroll") for (int r_ = 3; r_ < 15; r_ += 2) {                                                  \
                    mx_ = at_max3(mx_, s_acc[qb_][1][r_], s_acc[qb_][0][r_ + 1]);                                       \
                    mx_ = at_max3(mx_, s_acc[qb_][1][r_ + 1], s_acc[qb_][0][r_ + 2]);                                   \
                }                                                                                                       \
                mx_ = at_max3(mx_, s_acc[qb_][1][15], mx_);                                                             \
                mx_ = at_max3(mx_, __shfl_xor(mx_, 32, 64), mx_);                                                       \
                grow[qb_] = mx_ > m_run[qb_] + thr_x;                                                                   \
                const float mn_ = grow[qb_] ? mx_ : m_run[qb_];                                                         \
                alpha[qb_] = __builtin_amdgcn_exp2f((m_run[qb_] - mn_) * c_);                                           \
                m_run[qb_] = mn_;                                                                                       \
                const float mc_ = -mn_ * c_;                                                                            \
                float l0_ = 0.f, l1_ = 0.f;                                                                             \
                _Pragma("unroll") for (int kb_ = 0; kb_ < 2; kb_++)                                                     \
                _Pragma("unroll") for (int j_ = 0; j_ < 2; j_++)                                                        \
                _Pragma("unroll") for (int t_ = 0; t_ < 8; t_ += 2) {                                                   \
                    const float p0_ = __builtin_amdgcn_exp2f(__builtin_fmaf(s_acc[qb_][kb_][8 * j_ + t_], c_, mc_));    \
                    const float p1_ = __builtin_amdgcn_exp2f(__builtin_fmaf(s_acc[qb_][kb_][8 * j_ + t_ + 1], c_, mc_)); \
                    pf[qb_][kb_][j_][t_] = TR::from_f32(p0_);                                                           \
                    pf[qb_][kb_][j_][t_ + 1] = TR::from_f32(p1_);                                                       \
                    l0_ += p0_; l1_ += p1_;                                                                             \
                }                                                                                                       \
                l_run[qb_] = l_run[qb_] * alpha[qb_] + (l0_ + l1_);                                                     \
            } while (0)
#define A2_RESCALE(qb_) do {                                                                                           \
                if (__any(grow[qb_])) {                         /* some query of this block moved its maximum */        \
                    _Pragma("unroll") for (int d_ = 0; d_ < 2; d_++)                                                    \
                    _Pragma("unroll") for (int r_ = 0; r_ < 16; r_++) o_acc[qb_][d_][r_] *= alpha[qb_];                 \
                }                                                                                                       \
            } while (0)
            // ---- S^T for both query blocks (every K fragment feeds two MFMAs), softmax, P.V (every V^T fragment too) ----
#pragma unroll
            for (int qb = 0; qb < NQB; qb++)
#pragma unroll
                for (int kb = 0; kb < 2; kb++) A2_S_BIAS(qb, kb);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kb = 0; kb < 2; kb++) {
                const unsigned char *krow = s_k + (kb * 32 + l31) * AT2_ROW + (hi << 4);
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const V8 kf = *reinterpret_cast<const V8 *>(krow + (s << 5));
                    s_acc[0][kb] = TR::mfma(kf, qf[0][s], s_acc[0][kb]);
                    if (NQB == 2) s_acc[1][kb] = TR::mfma(kf, qf[1][s], s_acc[1][kb]);
                }
            }
            __builtin_amdgcn_s_setprio(0);
            // the bias registers are free: next tile's fragments land under the softmax / P.V of this one
            if (HAS_BIAS && more && !LATE) A2_FETCH_BIAS(kt + 1);
            if (LATE && more) A2_FETCH(kt + 1);
            A2_MASK(0);
            if (NQB == 2) A2_MASK(1);
            A2_SOFTMAX(0); A2_RESCALE(0);
            if (NQB == 2) { A2_SOFTMAX(1); A2_RESCALE(1); }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int d = 0; d < 2; d++) {
                const unsigned char *vrow = s_v + (d * 32 + l31) * AT2_ROW + (hi << 4);
#pragma unroll
                for (int kb = 0; kb < 2; kb++)
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        const V8 vf = *reinterpret_cast<const V8 *>(vrow + ((kb * 4 + j * 2) << 4));
                        o_acc[0][d] = TR::mfma(vf, pf[0][kb][j], o_acc[0][d]);
                        if (NQB == 2) o_acc[1][d] = TR::mfma(vf, pf[1][kb][j], o_acc[1][d]);
                    }
            }
            __builtin_amdgcn_s_setprio(0);
        }
        if (more) {
            A2_STASH1(cur ^ 1, st_row, kreg0, vreg0);
            A2_STASH1(cur ^ 1, st_row + 32, kreg1, vreg1);
        }
        __syncthreads();                                        // tile kt is read, tile kt + 1 is in place
    };
    const bool pad_keys = (P.n_valid & (AT_KB - 1)) != 0;
    for (int kt = 0; kt + 1 < ntiles; kt++) tile(kt, std::false_type());
    if (pad_keys) tile(ntiles - 1, std::true_type());
    else tile(ntiles - 1, std::false_type());
    if (!wave_live) return;
#pragma unroll
    for (int qb = 0; qb < NQB; qb++) {
        const float l_tot = l_run[qb] + __shfl_xor(l_run[qb], 32, 64);
        const float inv = 1.0f / l_tot;
        const int qrow = q0 + 32 * qb + l31;
        if (qrow < Np) {
            T *op = out_base + (size_t)qrow * (size_t)(H * AT_D);
#pragma unroll
            for (int d = 0; d < 2; d++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    T v4[4];
#pragma unroll
                    for (int t = 0; t < 4; t++) v4[t] = TR::from_f32(o_acc[qb][d][4 * g + t] * inv);
                    *reinterpret_cast<uint2 *>(op + d * 32 + 8 * g + 4 * hi) = *reinterpret_cast<const uint2 *>(v4);
                }
        }
    }
}

// bias operand: [H][Np/32][Np/64][4 chunks][64 lanes][8], values bias / scale (scale = 1/8: exact), saturated at the
// operand type's largest finite value: the bias MFMAs multiply this operand by an identity matrix, and an infinite entry times its
// zeros would turn the whole row NaN.  In float16 that is |bias| <= 8188 natural units -- a -1e4 "mask" entry stays a key with weight
// exp(-8188) = 0.
template <int BF16>
__global__ void k_attention_bias_pack2(const float *__restrict__ bias, typename at_traits<BF16>::T *__restrict__ out,
                                       int H, int n, int Np, float mul)
{
    typedef at_traits<BF16> TR;
    const long long total = (long long)H * Np * Np;
    const int n_kt = Np / AT_KB, nq32 = Np / 32;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int t = (int)(idx & 7), lane = (int)((idx >> 3) & 63), c = (int)((idx >> 9) & 3);
        const long long tile = idx >> 11;
        const int kt = (int)(tile % n_kt), qb = (int)((tile / n_kt) % nq32), h = (int)(tile / ((long long)n_kt * nq32));
        const int q = qb * 32 + 16 * (c & 1) + 8 * (lane >> 5) + t;
        const int k = kt * AT_KB + 32 * (c >> 1) + (lane & 31);
        const float v = (q < n && k < n) ? bias[((size_t)h * n + q) * n + k] * mul : 0.f;
        out[idx] = TR::from_f32(fminf(fmaxf(v, -TR::max_finite), TR::max_finite));
    }
}

// A/B switches of ds_attention_fwd, read once per process and again by ds_attention_reload_env (tests, A/B runs):
//   DS_ATT_GEN    0 / unset: generation by shape; 2: generation 2 everywhere; 4: generation 4 everywhere
//   DS_ATT_NQB    generation 2: 32-row query blocks per wave (1 or 2; unset: by sequence length)
//   DS_ATT_LATE   generation 2, 32 rows per wave: late K / V^T fetch (0 / 1; unset: on without a bias)
//   DS_ATT_ORDER  batch-fastest work order (0 / 1; unset: when one head's packed bias exceeds an L2)
//   DS_ATT_TAIL   query blocks with <= 4 live rows as GEMVs (ds_attention.h: at_tail_rows; 0 / 1, default 1)
struct AtEnv { int gen, nqb, late, order, tail; };
static AtEnv g_at_env = { -1, 0, -1, -1, 1 };
static void at_env_read()
{
    auto geti = [](const char *k, int d) { const char *v = getenv(k); return v && *v ? atoi(v) : d; };
    AtEnv e;
    e.gen = geti("DS_ATT_GEN", 0); e.nqb = geti("DS_ATT_NQB", 0); e.late = geti("DS_ATT_LATE", -1); e.order = geti("DS_ATT_ORDER", -1);
    e.tail = geti("DS_ATT_TAIL", 1);
    if (e.gen != 2 && e.gen != 4) e.gen = 0;
    g_at_env = e;
}
static const AtEnv &at_env()
{
    if (g_at_env.gen < 0) at_env_read();
    return g_at_env;
}
DS_API int ds_attention_reload_env(void)
{
    at_env_read();
    return DS_OK;
}

DS_API int ds_attention_bias_pack(ds_ctx *ctx, const float *bias, int H, int n, int Np, int dtype, void *packed, void *stream)
{
    DS_REQUIRE(ctx && bias && packed, DS_EINVAL, "ds_attention_bias_pack: null argument");
    DS_REQUIRE(H > 0 && n > 0 && Np >= n && (Np % 64) == 0, DS_EINVAL, "ds_attention_bias_pack: need 0 < n <= Np, Np a multiple of 64 (n %d, Np %d)", n, Np);
    DS_REQUIRE(dtype == DS_DTYPE_F16 || dtype == DS_DTYPE_BF16, DS_EINVAL, "ds_attention_bias_pack: dtype must be f16 or bf16");
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    const long long total = (long long)H * Np * Np;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 65536);
    hipStream_t st = (hipStream_t)stream;
    // A fragments of the bias MFMA, in units of 1/scale (head_dim 64: x 8, exact)
    if (dtype == DS_DTYPE_F16) hipLaunchKernelGGL((k_attention_bias_pack2<0>), dim3(blocks), dim3(256), 0, st, bias, (_Float16 *)packed, H, n, Np, 8.0f);
    else hipLaunchKernelGGL((k_attention_bias_pack2<1>), dim3(blocks), dim3(256), 0, st, bias, (__bf16 *)packed, H, n, Np, 8.0f);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}

// the three instantiations of one (dtype, bias) pair: late fetch exists for 32 rows per wave only
template <int BF16, int HAS_BIAS>
static void at2_launch(const AttnParams &P, int nqb, bool late, dim3 grid, hipStream_t st)
{
    if (nqb == 1 && late) hipLaunchKernelGGL((k_attention_fwd2<BF16, HAS_BIAS, 1, true>), grid, dim3(AT_THREADS), 0, st, P);
    else if (nqb == 1) hipLaunchKernelGGL((k_attention_fwd2<BF16, HAS_BIAS, 1, false>), grid, dim3(AT_THREADS), 0, st, P);
    else hipLaunchKernelGGL((k_attention_fwd2<BF16, HAS_BIAS, 2, false>), grid, dim3(AT_THREADS), 0, st, P);
}

DS_API int ds_attention_fwd(ds_ctx *ctx, const void *qk, const void *vt, const void *bias, void *out,
                            int B, int Np, int H, int n_valid, float scale, int dtype, void *stream)
{
    DS_REQUIRE(ctx && qk && vt && out, DS_EINVAL, "ds_attention_fwd: null argument");
    DS_REQUIRE(B > 0 && H > 0 && Np > 0 && (Np % 8) == 0, DS_EINVAL, "ds_attention_fwd: Np must be a positive multiple of 8 (got %d)", Np);
    DS_REQUIRE(n_valid > 0 && n_valid <= Np, DS_EINVAL, "ds_attention_fwd: n_valid %d outside 1..%d", n_valid, Np);
    DS_REQUIRE(dtype == DS_DTYPE_F16 || dtype == DS_DTYPE_BF16, DS_EINVAL, "ds_attention_fwd: dtype must be f16 or bf16");
    DS_REQUIRE((long long)B * H * ((Np + AT_QB - 1) / AT_QB) < (1ll << 30), DS_EUNSUPPORTED, "ds_attention_fwd: batch x heads too large for the grid");
    DS_REQUIRE(((uintptr_t)qk & 15) == 0 && ((uintptr_t)vt & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)bias & 15) == 0, DS_EINVAL,
               "ds_attention_fwd: operands must be 16-byte aligned");
    DS_HIP_CHECK(hipSetDevice(ctx->device));
    DS_REQUIRE(!bias || scale == 0.125f, DS_EUNSUPPORTED, "ds_attention_fwd: the packed bias is stored in units of 1/scale for "
               "head_dim 64 (scale 0.125); got scale %g", (double)scale);
    AttnParams P;
    P.qk = qk; P.vt = vt; P.bias = bias; P.out = out;
    P.B = B; P.Np = Np; P.H = H; P.n_valid = n_valid;
    P.c_exp = scale * 1.4426950408889634f;                                      // scale * log2(e)
    P.unused = 0.f;
    const AtEnv &E = at_env();
    // Where generation 4 (ds_attention4.hip: one wave per SIMD, two 32-query sub-blocks skewed inside the wave, 256 rows per
    // workgroup) is the default: nowhere.  Measured on the MI355X (profiles/round6_attention_gen4.txt, tools/att_ab.sh), f16, ms:
    //   (32, 1025, 16, bias) 0.283 generation 2 / 0.325 generation 4;  (8, 2443, 16) 0.282 / 0.281-0.303;  (8, 4097, 16, bias) 0.889 / 0.940;
    //   (32, 577, 12) 0.058 / 0.070;  (4, 1370, 16) 0.049 / 0.058.   DS_ATT_GEN=4 selects it (A/B runs, tests).
    // The two generations are bit-identical (same arithmetic per 32-query sub-block, another order of independent operations).
    const bool gen4 = (E.gen == 4);
    // rows per wave / 32.  Measured (f16, MI355X): 32 rows x 3 waves per SIMD wins on short sequences (N = 1025 + bias:
    // 0.286 vs 0.310 ms at batch 32; N = 577: 0.060 vs 0.076), 64 rows x 2 waves on long ones (N = 4097 + bias: 0.903 vs
    // 0.944; N = 2443: 0.255 vs 0.263); N = 1370 is a tie.  DS_ATT_NQB overrides (A/B runs).
    const int nqb = gen4 ? 2 : ((E.nqb == 1 || E.nqb == 2) ? E.nqb : (Np <= (bias ? 1280 : 2560) ? 1 : 2));
    // Late fetch (K / V^T of the next tile requested after S, 4 waves per SIMD) A/B on one box, 32 rows per wave:
    // N = 577: 0.064 -> 0.060, N = 1370: 0.404 -> 0.387, N = 2443: 0.272 -> 0.254 (vs 0.261 for 64 rows), no bias;
    // with bias it loses (N = 1025: 0.291 -> 0.300) and at N = 4097 64 rows per wave stay ahead (0.911 vs 0.946).
    // DS_ATT_LATE overrides.
    const bool late = (E.late >= 0 ? E.late : (bias ? 0 : 1)) != 0;
    // batch-fastest work order when one head's packed bias exceeds an L2 (see the kernel); DS_ATT_ORDER=0/1 overrides
    const int batch_fastest = E.order >= 0 ? E.order : (bias && B > 1 && (size_t)Np * Np * 2 > (size_t)(3u << 20) ? 1 : 0);
    P.flags = (batch_fastest ? 2 : 0) | (E.tail ? 4 : 0);
    P.nq = (Np + 128 * nqb - 1) / (128 * nqb);
    P.total = P.nq * H * B;
    P.chunk = (P.total + 7) / 8;
    const dim3 grid(8 * P.chunk);
    hipStream_t st = (hipStream_t)stream;
    const int kt = ds_kt_begin(ctx, DS_KT_ATTENTION, st);
    if (gen4) at4_launch(P, dtype == DS_DTYPE_BF16, bias != nullptr, grid, st);
    else if (dtype == DS_DTYPE_F16) { if (bias) at2_launch<0, 1>(P, nqb, late, grid, st); else at2_launch<0, 0>(P, nqb, late, grid, st); }
    else { if (bias) at2_launch<1, 1>(P, nqb, late, grid, st); else at2_launch<1, 0>(P, nqb, late, grid, st); }
    ds_kt_end(ctx, DS_KT_ATTENTION, kt, st);
    DS_HIP_CHECK(hipGetLastError());
    return DS_OK;
}
