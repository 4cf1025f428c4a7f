// The MFMA tile layouts of libnfx (v_mfma_f32_32x32x2_f32), each defined once. The pack, finish
// and assemble kernels turn an image offset into matrix coordinates with these functions, and the
// kernels that read an image take their index from them, so the two sides cannot disagree. To add
// a family, call these functions; do not spell the shifts out again. The static_asserts at the end
// are their test: the build fails if a layout stops being a bijection.
//
//   D[32 x 32] += A[32 x 2] * B[2 x 32]
//   A: lane l holds A[i = l & 31][k = l >> 5]       (weights, packed on device by *_pack)
//   B: lane l holds B[k = l >> 5][j = l & 31]       (activations, column j = one sample)
//   C/D: lane l, register r holds D[crow(r, l >> 5)][l & 31]
// Activations therefore live "hidden-unit rows x sample columns": a layer's accumulator tile
// is directly the B operand of the next layer (k-step (kt, r) reads register r of tile kt),
// with the weight operand permuted by the pack to match. No LDS round trip and no lane shuffles
// between layers.
#pragma once

#include <hip/hip_runtime.h>

namespace nfx {

// Row of register r in lane-half h of a 32x32 fp32 MFMA accumulator.
__host__ __device__ constexpr int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// Its inverse: the register and the lane half that hold row `row` (0..31).
__host__ __device__ constexpr int creg(int row) { return (row & 3) + 4 * (row >> 3); }
__host__ __device__ constexpr int chalf(int row) { return (row >> 2) & 1; }

struct RowCol {
    int row, col;
};

// ---- weight tiles, A-operand order [tile][rq][lane][rr], 1,024 floats per tile ----
// Lane l reads one f32x4 per rq: the weights of out row l & 31 for the k-steps 4 rq + rr, whose B
// operand is accumulator register 4 rq + rr of the layer below, i.e. contraction index
// crow(4 rq + rr, l >> 5).
struct ATileElem {
    int tile, row, k;  // tile number in the run; out row and contraction index inside the tile
};
// Decode: float offset t inside a run of tiles. The caller maps the tile number to (out tile,
// k tile): [ot][kt] images divide by the k-tile count, [kt][ot] images and the MADE (mu, alpha)
// pairs likewise with their own counts.
__host__ __device__ constexpr ATileElem a_tile_elem(int t) {
    const int rr = t & 3, lane = (t >> 2) & 63, rq = (t >> 8) & 3;
    return {t >> 10, lane & 31, crow(4 * rq + rr, lane >> 5)};
}
// Encode: tile number of (out tile ot, k tile kt) in an [ot][kt] image with NK k tiles, and the
// f32x4 index, in units of the 64 lanes, of quad rq of a tile.
__host__ __device__ constexpr int a_tile(int ot, int kt, int NK) { return ot * NK + kt; }
__host__ __device__ constexpr int a_quad(int tile, int rq) { return tile * 4 + rq; }
// Decode of a whole [ot][kt] image with NK k tiles: (out row, contraction column) of float offset t.
__host__ __device__ constexpr RowCol a_image_elem(int t, int NK) {
    const ATileElem e = a_tile_elem(t);
    return {32 * (e.tile / NK) + e.row, 32 * (e.tile % NK) + e.k};
}

// Layer-1 A operand [ht][ks][64] with KS1 k-steps: offset t holds W1[row][col], col = 2 ks + (l >> 5).
__host__ __device__ constexpr RowCol a1_elem(int t, int KS1) {
    const int lane = t & 63, ks = (t >> 6) % KS1, ht = (t >> 6) / KS1;
    return {32 * ht + (lane & 31), 2 * ks + (lane >> 5)};
}

// Per-row vectors (biases, W3 rows for VALU dots) in accumulator order [tile][lane half][16]:
// the row that offset t holds.
__host__ __device__ constexpr int acc_vec_row(int t) { return 32 * (t >> 5) + crow(t & 15, (t >> 4) & 1); }
// A run [n][HT][2][16] of such vectors, each over HT tiles (the rows of W3, the columns of W1,
// bias / gamma / beta): the vector that offset t lies in, and the row it holds.
struct VecRow {
    int vec, row;
};
__host__ __device__ constexpr VecRow acc_rows_elem(int t, int HT) {
    return {t / (32 * HT), acc_vec_row(t % (32 * HT))};
}

// ---- accumulator tiles dumped to memory, 1,024 values per tile ----
// [r][64] (register-major, lane-contiguous stores): the element at offset t, and the offset of
// element (row, col).
__host__ __device__ constexpr RowCol acc_dump_elem(int t) { return {crow(t >> 6, (t >> 5) & 1), t & 31}; }
__host__ __device__ constexpr int acc_dump_index(int row, int col) {
    return creg(row) * 64 + chalf(row) * 32 + col;
}
// [lane][16] (each lane stores its 16 registers as four f32x4): the element at offset t.
__host__ __device__ constexpr RowCol lane_dump_elem(int t) { return {crow(t & 15, (t >> 9) & 1), (t >> 4) & 31}; }

namespace tile_check {
constexpr bool crow_round_trips() {
    for (int row = 0; row < 32; ++row)
        if (crow(creg(row), chalf(row)) != row) return false;
    for (int r = 0; r < 16; ++r)
        for (int h = 0; h < 2; ++h)
            if (creg(crow(r, h)) != r || chalf(crow(r, h)) != h) return false;
    return true;
}
// offsets 0..1023 visit every (row, k) of tile 0 exactly once
constexpr bool a_tile_visits_all() {
    bool seen[32 * 32] = {};
    for (int t = 0; t < 1024; ++t) {
        const ATileElem e = a_tile_elem(t);
        if (e.tile != 0 || e.row < 0 || e.row > 31 || e.k < 0 || e.k > 31 || seen[e.row * 32 + e.k]) return false;
        seen[e.row * 32 + e.k] = true;
    }
    return true;
}
// the float a kernel reads as element rr of quad rq in lane l is the one the pack decoded
constexpr bool a_tile_encode_inverts() {
    for (int t = 0; t < 3 * 1024; ++t) {
        const ATileElem e = a_tile_elem(t);
        const int r = creg(e.k), lane = e.row + 32 * chalf(e.k);
        if ((a_quad(e.tile, r >> 2) * 64 + lane) * 4 + (r & 3) != t) return false;
    }
    return true;
}
// a 2 x 3 image: the float a kernel reads as element rr of quad rq of tile (ot, kt) in lane l is the
// one the pack decoded, and the decode stays inside the image
constexpr bool a_image_encode_inverts() {
    constexpr int NO = 2, NK = 3;
    for (int t = 0; t < NO * NK * 1024; ++t) {
        const RowCol e = a_image_elem(t, NK);
        if (e.row < 0 || e.row >= 32 * NO || e.col < 0 || e.col >= 32 * NK) return false;
        const int k = e.col & 31, r = creg(k), lane = (e.row & 31) + 32 * chalf(k);
        if ((a_quad(a_tile(e.row >> 5, e.col >> 5, NK), r >> 2) * 64 + lane) * 4 + (r & 3) != t) return false;
    }
    return true;
}
// three vectors over two tiles: load_bias16 of tile ht of vector n, lane half h, register r reads
// offset (n HT + ht) 32 + 16 h + r
constexpr bool acc_rows_encode_inverts() {
    constexpr int N = 3, HT = 2;
    for (int t = 0; t < N * HT * 32; ++t) {
        const VecRow e = acc_rows_elem(t, HT);
        if (e.vec < 0 || e.vec >= N || e.row < 0 || e.row >= 32 * HT) return false;
        if ((e.vec * HT + (e.row >> 5)) * 32 + 16 * chalf(e.row & 31) + creg(e.row & 31) != t) return false;
    }
    return true;
}
constexpr bool dumps_round_trip() {
    bool seen[32 * 32] = {};
    for (int t = 0; t < 1024; ++t) {
        const RowCol e = acc_dump_elem(t), l = lane_dump_elem(t);
        if (acc_dump_index(e.row, e.col) != t) return false;
        if (l.row < 0 || l.row > 31 || l.col < 0 || l.col > 31 || seen[l.row * 32 + l.col]) return false;
        seen[l.row * 32 + l.col] = true;
    }
    return true;
}
static_assert(crow_round_trips(), "creg/chalf invert crow for all 32 rows");
static_assert(a_tile_visits_all(), "A-operand decode is a bijection onto the tile");
static_assert(a_tile_encode_inverts(), "A-operand encode inverts the decode");
static_assert(a_image_encode_inverts(), "[ot][kt] image decode inverts the kernels' a_tile/a_quad index");
static_assert(acc_rows_encode_inverts(), "accumulator-order vector runs decode to the offset load_bias16 reads");
static_assert(dumps_round_trip(), "accumulator dump orders are bijections");
static_assert(acc_vec_row(32 + 16 + 5) == 32 + crow(5, 1), "accumulator-order vector");
}  // namespace tile_check

}  // namespace nfx
