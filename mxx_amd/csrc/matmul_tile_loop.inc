// matmul_tile_loop.inc — the accumulate loop of the register-tiled products (matmul_tile.h), included as text inside a
// kernel: acc[r][c][s] += A[r][k][s] * B[k][c][s] for k < inner, reduced once per `lazy` products.
//
// The including kernel has in scope
//   W, TR, TC, SV, NTB              its template parameters
//   VT, wxs, D                      TileTypes<W, SV>'s
//   D acc[TR][TC][SV]               the accumulators, cleared once (MXX_TILE_CLEAR)
//   uint32_t pending                products since the last reduction; it carries over from one inclusion's run to the next
//   const uint32_t lazy, inner      LimbConst::lazy_terms; the inner steps of this run
//   q, lc                           the limb's modulus and constants
// and defines, for this inclusion (both are undefined again here),
//   MXX_TILE_A(r, k)                const W *: the SV words of tile row r at inner step k
//   MXX_TILE_B(c, k)                const W *: the SV words of tile column c at inner step k
//   MXX_TILE_KU                     optionally: its own number of steps loaded ahead instead of kTileKU
#ifndef MXX_TILE_KU
#define MXX_TILE_KU (kTileKU<W, TR, TC, SV>)
#endif
{
    // the operands of KU steps are loaded before any of them is multiplied, so KU loads are in flight instead of one
    // (16 products (1 x 76)(76 x 4) at n = 256, L = 12: 0.46 -> 0.22 ms; M4 chain step 0.80 -> 0.73 ms).  The tail past
    // `inner` re-reads the last step and is dropped.
    constexpr uint32_t KU = MXX_TILE_KU;
    for (uint32_t k0 = 0; k0 < inner; k0 += KU) {
        W av[KU][TR][SV], bv[KU][TC][SV];
#pragma unroll
        for (uint32_t u = 0; u < KU; ++u) {
            const uint32_t k = min(k0 + u, inner - 1);
#pragma unroll
            for (int r = 0; r < TR; ++r) *reinterpret_cast<VT *>(av[u][r]) = *reinterpret_cast<const VT *>(MXX_TILE_A(r, k));
#pragma unroll
            for (int c = 0; c < TC; ++c) {
                // NTB (the host sets it when there is ONE row tile and B is beyond the Infinity Cache): B is streamed
                // exactly once and must not displace the left operands, which every column tile re-reads (matmul_kernel's
                // 32-bit branch has the figures).  A template flag: a run-time choice is merged into one plain load.
                const wxs *src = reinterpret_cast<const wxs *>(MXX_TILE_B(c, k));
                wxs t;
                if constexpr (NTB) t = __builtin_nontemporal_load(src);
                else t = *src;
#pragma unroll
                for (int s = 0; s < SV; ++s) bv[u][c][s] = t[s];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < KU; ++u) {
            if (KU > 1 && k0 + u >= inner) break;
#pragma unroll
            for (int r = 0; r < TR; ++r)
#pragma unroll
                for (int c = 0; c < TC; ++c)
#pragma unroll
                    for (int s = 0; s < SV; ++s) acc[r][c][s] += static_cast<D>(av[u][r][s]) * bv[u][c][s];
            if (++pending == lazy) {
                pending = 0;
#pragma unroll
                for (int r = 0; r < TR; ++r)
#pragma unroll
                    for (int c = 0; c < TC; ++c)
#pragma unroll
                        for (int s = 0; s < SV; ++s) acc[r][c][s] = tile_reduce<W>(acc[r][c][s], q, lc);
            }
        }
    }
}
#undef MXX_TILE_A
#undef MXX_TILE_B
#undef MXX_TILE_KU
