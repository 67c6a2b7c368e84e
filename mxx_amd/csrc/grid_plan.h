// grid_plan.h — the launch-grid arithmetic of the library, free of the HIP runtime.
//
// Every rule that turns a count of items, polynomials, limb vectors or tiles into the extents of a launch grid lives here,
// so that a plain C++ program can include it and check the rules over counts no device test can afford
// (tests/test_grid_plan_host.py).  Hardware limits: x <= 2^31 - 1 blocks, y and z <= 65535 each; HIP also rejects a launch
// with gridDim.x * blockDim.x >= 2^32.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
// the three extents of hip's dim3, for host programs built without the runtime
struct dim3 {
    uint32_t x, y, z;
    constexpr dim3(uint32_t x_ = 1, uint32_t y_ = 1, uint32_t z_ = 1) : x(x_), y(y_), z(z_) {}
};
#endif

// ---- one thread per item -----------------------------------------------------------------------
// HIP rejects launches with gridDim.x * blockDim.x >= 2^32 ("invalid configuration argument"), which a
// 64x1024 gadget matrix at n = 2^14 already exceeds: such kernels use item_grid() / item_index().
static inline dim3 item_grid(size_t items, unsigned threads) {
    const size_t blocks = (items + threads - 1) / threads;
    const size_t max_x = (static_cast<size_t>(1) << 31) / threads;
    if (blocks <= max_x) return dim3(static_cast<unsigned>(blocks ? blocks : 1));
    const size_t y = (blocks + max_x - 1) / max_x;
    return dim3(static_cast<unsigned>((blocks + y - 1) / y), static_cast<unsigned>(y));
}

// ---- one workgroup (row of workgroups along x) per entry ------------------------------------------
// The entry index is folded over y and z: the kernel rebuilds it as blockIdx.z * gridDim.y + blockIdx.y and returns when it
// is >= entries (the last z layer is ragged).  False: more than 65535 x 65535 entries, nothing to launch.  Every launcher
// of this shape calls it: the transpose, the column blocks, the Kronecker product, the preimage's gather / scatter, the
// target builders' combine, the three online lookups (both kernels of the slot-transfer evaluation) and the constant
// large-scalar kernel.  It is min(entries, 65535) and the rounded-up quotient, as those sites spelled it by hand, except
// at entries = 0 - which every site returns on before it gets here - where the hand-written form divided by zero and this
// one gives the 1 x 1 grid whose only block the guard sends back.
static inline bool fold_yz(size_t entries, size_t &gy, size_t &gz) {
    gy = std::min<size_t>(std::max<size_t>(entries, 1), 65535);
    gz = (entries + gy - 1) / gy;
    if (gz == 0) gz = 1;
    return gz <= 65535;
}

// grid of the grouped 2^14 kernels: (limb, poly) with the poly index split over y and z (each <= 65535)
static inline bool ntt14_grid(size_t vectors, uint32_t L, dim3 &grid) {
    if (L == 0 || vectors % L != 0) return false;
    const size_t polys = vectors / L;
    size_t z = (polys + 65534) / 65535;
    if (z == 0) z = 1;
    if (z > 65535 || polys % z != 0) {  // keep the grid exact (no out-of-range blocks): find a divisor split
        z = 0;
        for (size_t cand = (polys + 65534) / 65535; cand <= 65535 && cand <= polys; ++cand)
            if (polys % cand == 0 && polys / cand <= 65535) { z = cand; break; }
        if (z == 0) return false;
    }
    grid = dim3(L, static_cast<unsigned>(polys / z), static_cast<unsigned>(z));
    return true;
}

// the register-tiled products: the grid's y extent holds row tiles x column tiles
inline bool tile_grid_fits(uint64_t rows, uint64_t cols, uint32_t tr, uint32_t tc) {
    return ((rows + tr - 1) / tr) * ((cols + tc - 1) / tc) <= 65535;
}

// the gadget products' grid: x = chunks of a limb vector (each lane one 16-byte access per pass, up to four passes),
// (y, z) = limb vectors
struct VectorGrid {
    dim3 grid, block;
};
static inline VectorGrid vector_grid(uint32_t vectors, uint32_t N, uint32_t vn) {
    const uint32_t lanes = (N + vn - 1) / vn;  // accesses per limb vector
    const uint32_t threads = std::min<uint32_t>(256, (lanes + 63) / 64 * 64);
    const uint32_t per_block = threads * 4;
    const uint32_t gx = (lanes + per_block - 1) / per_block;
    const uint32_t gy = std::min<uint32_t>(vectors, 65535);
    const uint32_t gz = (vectors + gy - 1) / gy;  // vectors < 2^32 / 65535 * 65535: checked with the refusals
    return {dim3(gx, gy, gz), dim3(threads)};
}
constexpr uint64_t kMaxVectors = 65535ull * 65535ull;
