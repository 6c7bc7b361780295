// Tile primitives shared by the pre-split (hl32) LDS-DMA kernels: the big-tile forward / dgrad gather-GEMM
// (conv_hl_kernels.hip), its small-tile variants (conv_hlx_kernels.hip) and the weight-gradient kernels
// (wgrad_hl_kernels.hip, which shares the LDS-DMA load, kOob, the raw barrier and the MFMA burst only: its operands are
// pixel-major, with transposing reads and a swizzle key of their own).  What is stated here once: how a lane's LDS-DMA piece
// of the gathered operand is addressed (tile row -> pixel, source-side XOR swizzle, per-tap validity), the order in which the
// K stages walk (channel-chunk group, filter tap, chunk), the weight-piece and fragment offsets, and the three-product burst.
// The schedules -- phase tables, issue orders, counted waits -- are the kernels and stay in their files.
//
// Every function here is inlined into a kernel whose shared memory is ONE array (conv_hl_kernels.hip says why): helpers take
// LDS pointers as arguments and declare no __shared__ object.
#pragma once
#include "conv_shared.h"
#include "f16_split.h"

namespace dcnconv {

typedef __attribute__((address_space(3))) void* hl32_lds_ptr;

constexpr int kOob = (int)0x80000000;   // voffset that fails the bounds check of any buffer <= 2 GiB: LDS receives zeros

// LDS-DMA: 64 lanes x 16 B from rs[voffset + soffset] land at lds_dst + 16 lane
// (a NON-template function: inside a template this builtin breaks the host-side kernel stub with this compiler)
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t rs, void* lds_dst, int voffset, int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (hl32_lds_ptr)lds_dst, 16, voffset, soffset, 0, 0);
}

// raw s_barrier: no fence, LDS-DMA stays in flight across it
__device__ __forceinline__ void raw_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// Source-side XOR swizzle: the lane that fills PHYSICAL 16-byte slot ls of tile row `row` fetches this logical slot of the
// row's 128-byte hl32 line (conflict-free ds_read_b128 fragments, see hl32_foff)
__device__ __forceinline__ int hl32_src_slot(int row, int ls) { return ls ^ ((row >> 1) & 7); }

// Is the input pixel of filter-tap displacement (dy, dx) inside the image?  (by, bx): the pixel of tap (0, 0) -- output
// position -+ padding, stride 1.  TR: dgrad, the gather runs over the output gradient with mirrored taps.
template <bool TR>
__device__ __forceinline__ bool hl32_tap_inside(const GemmConv& p, int by, int bx, int dy, int dx) {
    if (TR) {
        const int ny = by - dy, nx = bx - dx;
        return ((ny | nx) >= 0) & (ny < p.hs) & (nx < p.ws);
    }
    return ((unsigned)(by + dy) < (unsigned)p.hs) & ((unsigned)(bx + dx) < (unsigned)p.ws);
}

// One lane's share of an LDS-DMA piece of the gathered operand (8 tile rows x 128 B; lane l: row l >> 3, physical slot l & 7).
struct Hl32Piece {
    int by, bx;       // pixel of tap (0, 0) of the lane's row
    int rowoff;       // byte offset of that pixel's line slot in the activation image
    unsigned vmask;   // MASK: one validity bit per filter tap (taps <= 32), else 0
};
// m0 + row: GEMM row of the lane (tile origin + tile row), ls: its physical slot, cs4: bytes per pixel of the activation image.
// MASK: the validity of the row under every filter tap as a word of bits (the traversal then forms the piece's offset when it
// is issued, Hl32KWalk::voffset_a); otherwise the caller tests the taps as it meets them (hl32_tap_inside on by, bx).
// Rows past M: every tap is invalid -- with a mask, the mask is empty (the rule of conv_hlx_kernels.hip, now also that of the
// 320-row tile); without one, `by` lies far outside the image, so that no tap brings it inside, and rowoff is 0.
template <bool TR, bool MASK>
__device__ __forceinline__ void hl32_piece(const GemmConv& p, int cs4, int m0, int row, int ls, Hl32Piece& q) {
    const int sl = hl32_src_slot(row, ls);
    const int m = m0 + row;
    const bool ok = m < p.M;
    const int mm = ok ? m : 0;
    const int img = fdiv(mm, p.div_hw), rem = mm - img * p.div_hw.d;
    const int y = fdiv(rem, p.div_w), x = rem - y * p.div_w.d;
    if constexpr (MASK) {
        const int by = TR ? y + p.pad : y - p.pad, bx = TR ? x + p.pad : x - p.pad;   // (stride 1)
        q.by = by;
        q.bx = bx;
        q.rowoff = (img * p.hs * p.ws + by * p.ws + bx) * cs4 + sl * 16;
        unsigned vm = 0u;
        const int taps = p.kh * p.kw;
        for (int tap = 0; tap < taps; ++tap) {
            const int r = fdiv(tap, p.div_kw), s = tap - r * p.kw;
            vm |= (hl32_tap_inside<TR>(p, by, bx, r * p.dil, s * p.dil) ? 1u : 0u) << tap;
        }
        q.vmask = ok ? vm : 0u;
    } else {
        q.by = ok ? (TR ? y + p.pad : y - p.pad) : -(1 << 28);
        q.bx = TR ? x + p.pad : x - p.pad;
        q.rowoff = ok ? (img * p.hs * p.ws + q.by * p.ws + q.bx) * cs4 + sl * 16 : 0;
        q.vmask = 0u;
    }
}

// K traversal: channel-chunk groups outermost (kcg chunks = up to 128 channels), then the filter taps, then the chunks of
// the group: the same input pixels come back for the next tap after kcg stages, while they are still in this XCD's L2.
// The state points at the 32-channel chunk whose LDS-DMA is issued next.
template <bool TR>
struct Hl32KWalk {
    int cs4;              // bytes per pixel of the activation image
    int cpt, kcg, taps;   // chunks per tap, chunks per group, filter taps
    int grp, tap, c;      // group, tap, chunk inside the group
    int delta, bit;       // displacement of the tap in bytes of the activation image (mirrored for TR), and the tap's bit of Hl32Piece::vmask

    // on_tap(dy, dx): the caller's share of a new filter tap (its displacement in pixels)
    template <class F>
    __device__ __forceinline__ void set_tap(const GemmConv& p, F on_tap) {
        const int r = fdiv(tap, p.div_kw), s = tap - r * p.kw;
        const int dy = r * p.dil, dx = s * p.dil;
        const int d = (dy * p.ws + dx) * cs4;
        delta = TR ? -d : d;
        bit = tap;
        on_tap(dy, dx);
    }
    template <class F>
    __device__ __forceinline__ void start(const GemmConv& p, int cs4_, int k0, F on_tap) {   // at chunk k0 of the traversal
        cs4 = cs4_;
        cpt = p.cs / 32;
        kcg = (cpt & 3) == 0 ? 4 : ((cpt & 1) == 0 ? 2 : 1);
        taps = p.kh * p.kw;
        const int per_grp = taps * kcg;
        grp = k0 / per_grp;
        const int rem = k0 - grp * per_grp;
        tap = rem / kcg;
        c = rem - tap * kcg;
        set_tap(p, on_tap);
    }
    // `step` chunks on (1, or the K groups of a small-tile stage: kcg is a multiple of it)
    template <class F>
    __device__ __forceinline__ void advance(const GemmConv& p, int step, F on_tap) {
        c += step;
        if (c >= kcg) {
            c = 0;
            if (++tap == taps) { tap = 0; ++grp; }
            set_tap(p, on_tap);
        }
    }
    // scalar offsets of the chunk: its line in a pixel of the activation image / in a row of the weight image
    __device__ __forceinline__ int soffset_a() const { return (grp * kcg + c) * 128; }
    __device__ __forceinline__ int soffset_b() const { return (tap * cpt + grp * kcg + c) * 128; }
    // voffset of a piece with a tap mask: formed when it is issued -- rowoff + the tap's (wave-uniform) displacement, or kOob
    __device__ __forceinline__ int voffset_a(const Hl32Piece& q) const { return ((q.vmask >> bit) & 1u) ? q.rowoff + delta : kOob; }
};

// voffset of a lane's share of a weight piece: row n (tile row `row`, physical slot ls) of the hl32 weight image [cd][nk lines]
__device__ __forceinline__ int hl32_vob(const GemmConv& p, int n, int row, int ls, int nk) {
    return n < p.cd ? n * (nk * 128) + hl32_src_slot(row, ls) * 16 : kOob;
}

// Fragment of v_mfma_f32_16x16x32_f16: lane (fr = lane & 15, fq = lane >> 4) holds k-octet fq of the stage's 32 k of row fr
// of a 16-row block.  Byte offset of the lane's 16-byte slot of plane pl (0 = hi, 1 = lo) inside the block's 16 lines.
__device__ __forceinline__ int hl32_foff(int lane, int pl) {
    const int fr = lane & 15, fq = lane >> 4, swz = (fr >> 1) & 7;
    return fr * 128 + ((pl * 4 + fq) ^ swz) * 16;
}

// The three-product burst of the split-fp16 arithmetic on TM x TN accumulator tiles acc[r0 + ..][c0 + ..]: product type
// outermost (the small cross terms lo x hi, hi x lo before hi x hi), the independent accumulators in between.
// fa / fb: [block][plane].  (The s_setprio bracket, where there is one, is the caller's.)
template <int TM, int TN, int ROWS, int COLS>
__device__ __forceinline__ void hl32_mfma3(const dcnsplit::h8 (*fa)[2], const dcnsplit::h8 (*fb)[2], f32x4_t (&acc)[ROWS][COLS],
                                           int r0, int c0) {
#pragma unroll
    for (int pt = 0; pt < 3; ++pt)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                acc[r0 + tm][c0 + tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pt == 0 ? fa[tm][1] : fa[tm][0],
                                                                               pt == 1 ? fb[tn][1] : fb[tn][0],
                                                                               acc[r0 + tm][c0 + tn], 0, 0, 0);
}

}  // namespace dcnconv
