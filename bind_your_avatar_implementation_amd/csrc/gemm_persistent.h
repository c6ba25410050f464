// What the persistent one-wave-per-SIMD kernels share AROUND their hand-placed K-loops: the XCD-contiguous group-M tile walk,
// the staging map, the buffer-descriptor and LDS-DMA helpers, the piece / fragment macro families, the launcher tail -- and
// the description of the LDS image of a K-tile that staging, fragment reads and epilogues have to agree on.
// Users: gemm_v4.hip (256 x 256 bf16), gemm_v5.hip / gemm_v6.hip (128 x 256 bf16), gemm_fp8_v4.hip (256 x 256 e4m3),
// gemm_mx_v4.hip (256 x 256 e4m3 with e8m0 block scales), attn_w4.hip
// (descriptors, LDS-DMA, XCD range) and attn.hip (XCD range).  The K-loops, their schedules and their rings stay in those files.
//
// THE LDS IMAGE OF A K-TILE (the contract between staging, fragment reads and gemm_wide_epilogue.h -- written down here only)
//
//  * A K-tile of an operand is `rows` LDS rows of 128 BYTES: 64 bf16 or 128 e4m3 values of one matrix row.  A row is eight
//    16-byte chunks; chunk c of row `row` sits at chunk position  c ^ ((row >> 1) & 7): the 16 lanes of a
//    ds_read_b128 quarter-wave read the same chunk of 16 consecutive rows, and the XOR spreads them over all banks.
//  * The swizzle is applied on the SOURCE side.  An LDS-DMA piece writes 1 KiB linearly -- lane l's 16 bytes go to row
//    l >> 3, chunk position l & 7 of the piece's eight rows -- so the lane LOADS the chunk that belongs there:
//    (l & 7) ^ ((row >> 1) & 7)  (stage_off).  Per-lane source offsets are relative to the tile origin and never change;
//    the origin lives in the buffer descriptor (a_rsrc / w_rsrc of the kernels: base advanced to the tile's first row, size =
//    what is left of the matrix), so rows past M / N arrive as zeros and a past-the-end tile has an empty descriptor.
//  * A rows are staged in order: LDS row = tile row.  W rows are staged PERMUTED: LDS slot row  s = 128 h + 16 i + r
//    (h: which wave column, i = 0..7: the wave's accumulator column block, r = 0..15: the MFMA's column lane) holds tile
//    column  128 h + ((r & 3) * 4 + (r >> 2)) * 8 + i  (w_slot_col).  The 16x16 accumulator block i of a lane (fr, fq),
//    register e, is MFMA column r = 4 fq + e, i.e. output column  n_wave + (4 e + fq) * 8 + i:  over i = 0..7 a lane
//    holds EIGHT CONSECUTIVE output columns, and the epilogues of gemm_wide_epilogue.h read bias / gate / residual and
//    write C sixteen bytes per lane.
//  * Fragments: the lane (fr = lane & 15, fq = lane >> 4) reads chunk fq (k-step 0) and chunk 4 + fq (k-step 1) of row
//    row0 + fr; row blocks are 16 rows = 2048 bytes apart (the ds_read's immediate offset).  The e4m3 kernel's one
//    k-step takes both chunks as the low and high half of its 32 operand bytes.
//
// THE 64-BYTE-ROW IMAGE (e2m1 weights of gemm_mx_v4.hip: 128 four-bit values of one matrix row per K-tile)
//
//  * A K-tile of the operand is `rows` LDS rows of 64 BYTES back to back: four 16-byte chunks = the four 32-element MX blocks
//    of the row.  Chunk c of row `row` sits at chunk position  c ^ (((row >> 2) & 1) << 1)  -- the image of a 16-row block is
//    the tiled kernel's (stage_mx<MX_E2M1> / lds_frag_mx<MX_E2M1>, gemm_mx.hip): unswizzled, the rows of a ds_read_b128 lane
//    group would meet two to a 16-byte slot of the 256-byte bank row; with the XOR each group covers the 16 slots once.
//  * Source-side swizzle again: a piece writes 1 KiB linearly = SIXTEEN rows, lane l's 16 bytes to row l >> 2, chunk position
//    l & 3, so the lane loads chunk  (l & 3) ^ (((row >> 2) & 1) << 1)  (stage_off64).  K-tile t is bytes [64 t, 64 t + 64) of
//    a source row; the descriptor's extent ends K / 2 bytes into the last row (tile_rsrc_w's row_bytes).
//  * Rows are staged through the SAME slot permutation (w_slot_col), so the accumulator layout and the epilogues do not change.
//  * Fragments: the lane (fr, fq) reads chunk fq -- block fq, low nibble first, the four-register e2m1 operand of the
//    block-scaled MFMA -- of row row0 + fr: ONE ds_read_b128; row blocks are 16 rows = 1024 bytes apart (frag_addr64).
//
// THE 96-BYTE-ROW IMAGE (e2m3 operands of gemm_mx_v4.hip: 128 six-bit values of one matrix row per K-tile)
//
//  * A K-tile of the operand is `rows` LDS rows of 96 BYTES back to back: four 24-byte MX blocks.  Rows whose bit 3 is set
//    are ROTATED by half a row: byte b of source row `row` sits at byte  (b + 48 s) % 96,  s = (row >> 3) & 1, i.e. block c at
//    block position  c ^ 2 s.  (The tiled kernel swaps 16-byte chunk pairs instead -- stage_mx<MX_E2M3>, gemm_mx.hip -- which
//    cuts a lane's 24 bytes in two: three addresses per lane.  Rotating by two whole blocks keeps them together: ONE.)
//  * Banks (MI355X: a ds_read_b64 is served in two groups of 32 lanes, bank = (address / 4) mod 64, 8 bytes = 2 banks per lane,
//    so a group is conflict-free exactly when its 32 lanes cover the 64 banks once).  A group is the 16 rows fr of two blocks
//    fq = 2 g, 2 g + 1.  Row r starts at dword 24 r: 24 r mod 64 runs over the eight multiples of 8 for r = 0..7, and again
//    for r = 8..15 -- unrotated, rows r and r + 8 would meet in every bank (2-way on every read).  Read p = 0..2 of the lane
//    takes dwords 24 r + 6 (fq ^ 2 s) + 2 p + {0, 1}.  Every base 24 r mod 64 belongs to one row with s = 0 and one with s = 1,
//    so the group covers the 64 banks once exactly when the eight dword offsets it adds to a base differ mod 8: they are
//    2 p + {0, 1, 6, 7} (s = 0) and 2 p + {12, 13, 18, 19} (s = 1), mod 8 the residues 2 p + {0, 1, 6, 7, 4, 5, 2, 3} (the
//    second group, fq = 2, 3, is the first shifted by 12 dwords).  Three conflict-free ds_read_b64 per fragment: 6 LDS cycles
//    for 1536 bytes, the array's full 256 bytes per clock.
//  * Source-side rotation: a wave's 64 rows are 6 KiB = SIX linear 1-KiB pieces; lane l of piece q writes bytes
//    t .. t + 15, t = 1024 q + 16 l, of the wave's share = row t / 96, byte b = t % 96 (a multiple of 16, as is 48), so it
//    LOADS source bytes  (b + 48 s) % 96 .. + 15  of that row: one aligned 16-byte chunk that never wraps (stage_off96).
//    K-tile t is bytes [96 t, 96 t + 96) of a source row; the descriptor's extent ends 3 K / 4 bytes into the last row.
//  * W rows go through the SAME slot permutation (w_slot_col): accumulator layout and epilogues do not change.
//  * Fragments: the lane (fr, fq) reads the 24 bytes at block position fq ^ 2 s of row row0 + fr -- block fq, element i at bits
//    6 i.., the six-register e2m3 operand of the block-scaled MFMA -- as three ds_read_b64 at +0, +8, +16; row blocks are 16
//    rows = 1536 bytes apart, which leaves s = fr >> 3 alone (frag_addr96).
#pragma once
#include "gemm_common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- the tile walk -------------------------------------------------------------------------------------------------------
// XCD x (= blockIdx % 8 under round-robin dispatch; speed only) owns the contiguous range [base, end) of an order of `total`
// items: what its workgroups have in flight at any moment then shares panels through that XCD's L2.
struct XcdRange { int base, end; };
__host__ __device__ __forceinline__ XcdRange xcd_range(int total, int xcd) {
    const int cq = total >> 3, cr = total & 7;
    const int base = (xcd < cr) ? xcd * (cq + 1) : cr * (cq + 1) + (xcd - cr) * cq;
    return {base, base + cq + (xcd < cr ? 1 : 0)};
}

struct PersistentTile { int z, m0, n0; bool valid; };

// The output tiles of one workgroup: its XCD's range of the group-M order, of which the XCD's `slots` workgroups take every
// slots-th tile, round after round.  Group-M order: gm row tiles sweep a column tile before the order moves on -- what the
// concurrent tiles of an XCD share in its L2 (gm per shape: gemm_group_m, gemm_common.h; the sweep behind it: gemm_v4.hip).
template <int BM, int BN>
struct TileWalk {
    int tiles_m, tiles_n, per_z, gm;
    int base, end, slot, slots;
    __device__ __forceinline__ TileWalk(int tiles_m_, int tiles_n_, int batch, int gm_)
        : tiles_m(tiles_m_), tiles_n(tiles_n_), per_z(tiles_m_ * tiles_n_), gm(gm_) {
        const int total = per_z * batch, xcd = blockIdx.x & 7;
        slot = blockIdx.x >> 3;
        slots = gridDim.x >> 3;
        const XcdRange r = xcd_range(total, xcd);
        base = r.base;
        end = r.end;
    }
    // the seq-th tile of this workgroup; past the end: invalid, with the coordinates of `base` (its descriptors are empty,
    // nothing is stored)
    __device__ __forceinline__ PersistentTile coord(int seq) const {
        PersistentTile c;
        const int id = base + slot + seq * slots;
        c.valid = id < end;
        const int idz = c.valid ? id : base;
        c.z = idz / per_z;
        const int idt = idz - c.z * per_z;
        const int per_group = gm * tiles_n;
        const int group = idt / per_group, first_m = group * gm;
        const int gsz = (tiles_m - first_m) < gm ? (tiles_m - first_m) : gm;
        const int in_g = idt - group * per_group;
        c.m0 = (first_m + in_g % gsz) * BM;
        c.n0 = (in_g / gsz) * BN;
        return c;
    }
};

// ---- the staging map (see the top) ------------------------------------------------------------------------------------------
// tile column held by W slot row s
__device__ __forceinline__ int w_slot_col(int s) {
    const int r = s & 15, i = (s >> 4) & 7;
    return (s & 128) + (((r & 3) << 2) | (r >> 2)) * 8 + i;
}
// byte offset, from the tile origin, of what `lane` moves to LDS row rl of its piece: the swizzled chunk of source row (A) or
// source column (W) src_row; pitch = bytes between them (lda * 2 for bf16, lda for e4m3)
__device__ __forceinline__ uint32_t stage_off(int lane, int rl, int src_row, uint32_t pitch) {
    return (uint32_t)src_row * pitch + ((lane & 7) ^ ((rl >> 1) & 7)) * 16;
}

// ... and of the 64-byte-row image: `lane` moves 16 bytes to LDS row rl (= piece row lane >> 2), chunk position lane & 3
__device__ __forceinline__ uint32_t stage_off64(int lane, int rl, int src_row, uint32_t pitch) {
    return (uint32_t)src_row * pitch + ((lane & 3) ^ (((rl >> 2) & 1) << 1)) * 16;
}

// ... and of the 96-byte-row image: `lane` moves 16 bytes of piece q (0..5) of a wave's 64 rows.  stage_row96: the row, 0..63,
// inside the wave's share; stage_off96: the offset, for that row as LDS row rl (its bit 3 decides the rotation)
__device__ __forceinline__ int stage_row96(int lane, int q) { return (q * 1024 + lane * 16) / 96; }
__device__ __forceinline__ uint32_t stage_off96(int lane, int q, int rl, int src_row, uint32_t pitch) {
    const int b = (q * 1024 + lane * 16) % 96;
    return (uint32_t)src_row * pitch + (uint32_t)((b + 48 * ((rl >> 3) & 1)) % 96);
}

// ---- buffer descriptors and LDS-DMA --------------------------------------------------------------------------------------
__device__ __forceinline__ i32x4 raw_rsrc(const void* base, uint32_t bytes) {
    const unsigned long long b = (unsigned long long)base;
    i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffu));
    r.y = __builtin_amdgcn_readfirstlane((int)((b >> 32) & 0xffffu));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}

// one 1-KiB LDS-DMA piece: 64 lanes x 16 bytes from per-lane global offsets to LDS [m0 .. m0 + 1024)
template <int LDS_OFF = 0>
__device__ __forceinline__ void dma_piece(uint32_t lds_base, uint32_t voff, const i32x4& rsrc, uint32_t soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :
                 : "s"(lds_base + LDS_OFF), "v"(voff), "s"(rsrc), "s"(soff)
                 : "memory");
}

// A / W of tile c behind its origin: what is left of the matrix (T: bf16_t or a byte type for e4m3), nothing for an invalid tile
// row_elems: as tile_rsrc_w's (e2m3 codes: 3 K / 4 bytes)
template <typename T>
__device__ __forceinline__ i32x4 tile_rsrc_a(const GemmArgs& p, const T* A, const PersistentTile& c, int row_elems = 0) {
    const long long left = ((long long)(p.M - 1 - c.m0) * p.lda + (row_elems ? row_elems : p.K)) * (long long)sizeof(T);
    return raw_rsrc(A + (long long)c.z * p.a_bs + (long long)c.m0 * p.lda, c.valid && left > 0 ? (uint32_t)left : 0u);
}
// row_elems: elements of T that the GEMM reads of a W row where that is not K (e2m1 codes: K / 2 bytes); 0 = K
template <typename T>
__device__ __forceinline__ i32x4 tile_rsrc_w(const GemmArgs& p, const T* W, const PersistentTile& c, int row_elems = 0) {
    const long long left = ((long long)(p.N - 1 - c.n0) * p.ldw + (row_elems ? row_elems : p.K)) * (long long)sizeof(T);
    return raw_rsrc(W + (long long)c.n0 * p.ldw, c.valid && left > 0 ? (uint32_t)left : 0u);
}

// LDS address of 16-byte chunk `chunk` of row `row` of the operand tile at `tile`: a lane's fragments are chunk fq (k-step 0)
// and chunk 4 + fq (k-step 1) of row row0 + fr
__device__ __forceinline__ uint32_t frag_addr(uint32_t tile, int row, int chunk) {
    return tile + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// ... of the 64-byte-row image: the lane's one fragment is chunk fq of row row0 + fr
__device__ __forceinline__ uint32_t frag_addr64(uint32_t tile, int row, int chunk) {
    return tile + row * 64 + ((chunk ^ (((row >> 2) & 1) << 1)) << 4);
}

// ... of the 96-byte-row image: the lane's one fragment is the 24 bytes at block position fq ^ 2 s of row row0 + fr
__device__ __forceinline__ uint32_t frag_addr96(uint32_t tile, int row, int blk) {
    return tile + row * 96 + (blk ^ (((row >> 3) & 1) << 1)) * 24;
}

// piece Q of a wave's share (1 KiB apart in LDS), per-lane offsets VO[Q]
#define DMA_PIECE(Q, BASE, VO, RS, SOFF) dma_piece<(Q) * 1024>(BASE, VO[Q], RS, SOFF)
#define ALL4(M, ...) M(0, __VA_ARGS__); M(1, __VA_ARGS__); M(2, __VA_ARGS__); M(3, __VA_ARGS__)
#define ALL6(M, ...) ALL4(M, __VA_ARGS__); M(4, __VA_ARGS__); M(5, __VA_ARGS__)
#define ALL8(M, ...) ALL4(M, __VA_ARGS__); M(4, __VA_ARGS__); M(5, __VA_ARGS__); M(6, __VA_ARGS__); M(7, __VA_ARGS__)
// Inline-asm MFMAs are invisible to hipcc: nothing tells it that an LDS return must not land in a register a queued MFMA still
// has to read, so every fragment stays allocated to its fragment to the end of the K-tile (F: an array of 4 / 8 fragments)
#define KEEP4(F) asm volatile("" :: "v"(F[0]), "v"(F[1]), "v"(F[2]), "v"(F[3]))
#define KEEP8(F) asm volatile("" :: "v"(F[0]), "v"(F[1]), "v"(F[2]), "v"(F[3]), "v"(F[4]), "v"(F[5]), "v"(F[6]), "v"(F[7]))

// ---- host side: one workgroup per CU, whole rounds of the eight XCDs when the tiles do not fill the 256 CUs
inline int persistent_grid(long long total) { return (int)(total < 256 ? (total + 7) / 8 * 8 : 256); }

// launch KERNEL with `lds` bytes of dynamic LDS (above the 64 KiB default: raised once per kernel and device)
template <auto KERNEL, typename... Args>
int launch_persistent(int blocks, int threads, size_t lds, hipStream_t s, const Args&... args) {
    static std::atomic<unsigned long long> attr_done{0};
    if (bya_allow_big_lds(reinterpret_cast<const void*>(KERNEL), (int)lds, attr_done) != BYA_OK) return BYA_ERR_LAUNCH;
    BYA_LAUNCH(KERNEL, dim3(blocks), dim3(threads), lds, s, args...);
    return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
}

}  // namespace
