// path_large_layout.hpp -- where the launch-per-iteration drivers (path_large.hip) keep what: every region of PathArgs::work,
// PathArgs::sympk, WideArgs::scratch and SpwArgs::vec is named HERE, once; the drivers take their pointers from these structs and
// the allocation sizes (path_large_work_doubles, sympk_doubles, wide_scratch_doubles, spw_vec_doubles) are their totals.
//
// Plain C++: no HIP, so that a host compiler alone can print the tables (tests/test_launch_workspace_cpu.py holds them to
// tests/golden/launch_workspace.json).  Offsets and lengths are counted in DOUBLES from the start of the buffer; regions follow each
// other without gaps in the order of their fields (spare doubles are part of the region in front of them).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OEM_LAYOUT_HD __host__ __device__
#else
#define OEM_LAYOUT_HD
#endif

namespace oemgpu {

constexpr int STATE_DBL = 16;                   // the path state (LState) in front of PathArgs::work
constexpr int MAXL = 512;                       // Lanczos steps kept
constexpr int FMAXB = 1024;                     // flag words per launch parity
constexpr int SYM_TB = 128;                     // edge of a symmetric tile / of a packed block
constexpr int SPK_TILE = SYM_TB * SYM_TB;       // doubles of a packed block (128 KiB)
constexpr int SPK_HC = 32;                      // coordinates per workgroup of the packed products' slot sum and head
constexpr int SPW_T_DOUBLES = 2 * MAXL;         // the Lanczos table behind the sparse wide engine's vectors

struct Region {
    size_t off, len;
    size_t end() const { return off + len; }
};
// lays regions end to end
struct RegionCursor {
    size_t at = 0;
    Region take(size_t len) { Region r{at, len}; at += len; return r; }
};

// ---- PathArgs::work of run_path_large (the p >= n drivers use its head: state | beta | g)
struct LargeWork {
    Region state;                   // LState
    Region beta, g, v, vp, w;       // q + 8 each: the iterate, the product, the Lanczos vectors
    Region T;                       // alpha[MAXL] | beta[MAXL] | 64 spare
    Region fstate, fdone;           // fused engine: FState[2] | the done word
    Region Bv, flags;               // ... beta[2][q + 8] (shared with the replicated engine) | flags[2][FMAXB] ints
    Region gstate, Uv;              // replicated-update engine: GState[2] | u[2][q + 8]
    Region Vc, Vp, Wb;              // fused Lanczos: two copies each of v, v_prev, w
    Region sym_part, sym_state;     // symmetric-tile engine (q = 4096): partial vectors P[2][q / 128][q] | SState[2]
    Region uf;                      // U[q] | F[ngroups <= q] of path_update_kernel where they do not fit its LDS
    size_t total;
};
inline LargeWork large_work(int q)
{
    const size_t v = (size_t)q + 8;
    const bool sym = q == 4096;
    RegionCursor c;
    LargeWork L;
    L.state = c.take(STATE_DBL);
    L.beta = c.take(v); L.g = c.take(v); L.v = c.take(v); L.vp = c.take(v); L.w = c.take(v);
    L.T = c.take(2 * MAXL + 64);
    L.fstate = c.take(8); L.fdone = c.take(8);
    L.Bv = c.take(2 * v); L.flags = c.take(FMAXB);
    L.gstate = c.take(16); L.Uv = c.take(2 * v);
    L.Vc = c.take(2 * v); L.Vp = c.take(2 * v); L.Wb = c.take(2 * v);
    L.sym_part = c.take(sym ? 2 * (size_t)(q / SYM_TB) * q : 0); L.sym_state = c.take(sym ? 16 : 0);
    L.uf = c.take(2 * v);
    L.total = c.at;
    return L;
}

// ---- PathArgs::sympk (q > 1024): the packed lower triangle of XX and what its products and the (head, product) pairs keep behind it
OEM_LAYOUT_HD inline int spk_nblk(int q) { return (q + SYM_TB - 1) / SYM_TB; }
OEM_LAYOUT_HD inline size_t spk_ntile(int q) { const size_t nb = (size_t)spk_nblk(q); return nb * (nb + 1) / 2; }
struct SpkWork {
    int nblk, qpad, ntile;          // blocks per edge, q rounded up to whole blocks, blocks of the triangle
    Region blocks;                  // ntile packed blocks
    Region P;                       // partial vectors P[nblk][qpad]
    Region B;                       // B[2][qpad]: the iterate by launch parity
    Region flags;                   // flags[2][FMAXB] ints
    Region sstate, done;            // SState[2] | the done word
    Region nz32;                    // nz32[2][qpad / 32] ints: which 32-coordinate pieces of B[parity] hold a non-zero | 8 spare
    Region gen;                     // the head's parts of the sums over all coordinates [4][FMAXB] + its state words [2][4]
    size_t total;                   // 0 for q <= 1024
    size_t zero_from, zero_doubles; // what is cleared before the first product: everything from B on
};
inline SpkWork spk_work(int q)
{
    SpkWork S{};
    if (q <= 1024) return S;
    S.nblk = spk_nblk(q); S.qpad = S.nblk * SYM_TB; S.ntile = (int)spk_ntile(q);
    const size_t qpad = (size_t)S.qpad;
    RegionCursor c;
    S.blocks = c.take((size_t)S.ntile * SPK_TILE);
    S.P = c.take((size_t)S.nblk * qpad);
    S.B = c.take(2 * qpad);
    S.flags = c.take(FMAXB);
    S.sstate = c.take(16); S.done = c.take(8);
    S.nz32 = c.take(qpad / 32 + 8);
    S.gen = c.take(4 * FMAXB + 16);
    S.total = c.at;
    S.zero_from = S.B.off; S.zero_doubles = S.total - S.B.off;
    return S;
}

// ---- p >= n: the standardised copy's row blocks, the workgroups of the column kernels, and WideArgs::scratch
// `nb` row blocks of `rb` rows each (the last may hold fewer), every block a column-major (64 nr) x p matrix of its own with zero
// padding rows -- a column of a block lives in the registers of one wave (nr <= 32 doubles per lane).  n <= 2048: one block.
struct WideLayout {
    int nb;                  // row blocks
    int rb;                  // data rows per block (block b holds rows [b rb, min(n, (b + 1) rb)))
    int nr;                  // 64-row register slices per block: a block has 64 nr rows
    OEM_LAYOUT_HD long long npad() const { return 64LL * nr; }              // rows of one block
    OEM_LAYOUT_HD long long rows() const { return (long long)nb * 64 * nr; }  // rows of all blocks (vectors of this length)
};
inline int wide_nr(int n)
{
    const int sizes[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};
    const int need = (n + 63) / 64;
    for (int v : sizes) if (v >= need) return v;
    return 0;
}
// waves per workgroup: as many as the combine buffer in LDS (NW x 64 NR doubles <= 64 KB) and the registers (3-4 NR doubles per
// lane) allow -- a wave walks its columns one after the other (dot product -> wave sum -> operator -> update is a serial chain of
// ~400 cycles per column), so the CU needs several waves per SIMD to keep loads in flight
OEM_LAYOUT_HD constexpr int wide_nw(int nr) { return nr <= 8 ? 16 : (nr <= 16 ? 8 : 4); }
inline WideLayout wide_layout(int64_t n)
{
    WideLayout L;
    L.nb = n <= 2048 ? 1 : (int)((n + 2047) / 2048);
    L.rb = (int)((n + L.nb - 1) / L.nb);
    L.nr = wide_nr(L.rb);
    return L;
}
inline int wide_workgroups(int n, int p)
{
    const int nw = wide_nw(wide_layout(n).nr);
    int w = (p + nw - 1) / nw;                           // small p is latency-bound: a column per wave, as many CUs as that gives
    if (w > 256) w = 256;                                // one workgroup per CU: every partial vector is read back by the reduction
    return w < 1 ? 1 : w;
}
struct WideScratch {
    Region P;                      // partial vectors P[W][npad()]
    Region r, t, v, vp, w;          // rows() each: residual (one row block only), Xs beta, the Lanczos vectors
    Region T;                       // alpha[MAXL] | beta[MAXL] | 64 spare
    Region sstate, done;            // SState[2] | the done word (2)
    Region flags;                   // flags[2][FMAXB] ints | 64 spare
    Region gb;                      // gb[nb][p + 8]: the row blocks' parts of g
    size_t own_total;               // (the scratch also holds the persistent engines' exchange buffers: wide_scratch_doubles)
};
inline WideScratch wide_scratch(int n, int p, int W, const WideLayout &lay)
{
    (void)n;
    const size_t rows = (size_t)lay.rows();
    RegionCursor c;
    WideScratch S;
    S.P = c.take((size_t)W * (size_t)lay.npad());
    S.r = c.take(rows); S.t = c.take(rows); S.v = c.take(rows); S.vp = c.take(rows); S.w = c.take(rows);
    S.T = c.take(2 * MAXL + 64);
    S.sstate = c.take(16); S.done = c.take(2);
    S.flags = c.take(FMAXB + 64);
    S.gb = c.take((size_t)lay.nb * ((size_t)p + 8));
    S.own_total = c.at;
    return S;
}

// ---- SpwArgs::vec of the sparse wide engine: t | v | v_prev | w (n doubles each) | the Lanczos table
struct SpwVec {
    Region t, v, vp, w, T;
    size_t total;
};
inline SpwVec spw_vec(int64_t n)
{
    RegionCursor c;
    SpwVec V;
    V.t = c.take((size_t)n); V.v = c.take((size_t)n); V.vp = c.take((size_t)n); V.w = c.take((size_t)n);
    V.T = c.take(SPW_T_DOUBLES);
    V.total = c.at;
    return V;
}
inline size_t spw_vec_doubles(int64_t n) { return spw_vec(n).total; }

}  // namespace oemgpu
