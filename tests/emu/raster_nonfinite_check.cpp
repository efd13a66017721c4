// raster_nonfinite_check.cpp -- stand-alone check of the rasteriser forward on non-finite and overflowing splats (DESIGN.md
// "Parity"), through the C ABI of the emulator build of the kernel sources.  TEST INFRASTRUCTURE ONLY: built and run by
// tests/test_raster_forward_edges.py against tests/emu/_build/libgs2mesh_emu.so; for a sanitizer run, compile it together with
// the kernel sources and emu_runtime.cpp under -fsanitize=address,undefined,float-cast-overflow.
// A 64 x 32 view, an 8 x 5 grid of ordinary splats, and one bad splat of each kind in tile (0, 0) and in tile (2, 1), rendered at
// cull levels 0, 1, 2 with blend variants 0 and 4 and 16 x 16 / 16 x 32 binning tiles.  Checked: no call fails, no radius is
// negative, the lists did not overflow, and every pixel outside the tiles of the bad splats equals the render without them.
// Exit status 0 and "ok" = every case passed.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gs2mesh_amd.h"

static int g_failed = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                              \
        }                                                            \
    } while (0)

static const int W = 64, H = 32;
static const float F = 64.0f;

struct Model {
    std::vector<float> xyz, scale, rot, op, col;
    int P() const { return (int)op.size(); }
    void add(float u, float v, float z, float s, float o) {
        xyz.push_back((u - 0.5f * (W - 1)) * z / F);
        xyz.push_back((v - 0.5f * (H - 1)) * z / F);
        xyz.push_back(z);
        for (int k = 0; k < 3; ++k) scale.push_back(s);
        const float q[4] = {1.0f, 0.0f, 0.0f, 0.0f};
        rot.insert(rot.end(), q, q + 4);
        op.push_back(o);
        const int i = P();
        col.push_back(0.1f * (float)(i % 10));
        col.push_back(0.13f * (float)(i % 7));
        col.push_back(0.2f * (float)(i % 5));
    }
};

// the last splat of the model becomes bad splat number `kind`; returns 0 past the last kind
static int spoil(Model& m, int kind) {
    const int i = m.P() - 1;
    const float nan = NAN, inf = INFINITY;
    switch (kind) {
        case 0: m.scale[3 * i + 1] = nan; break;
        case 1: m.scale[3 * i + 1] = inf; break;
        case 2: m.rot[4 * i + 2] = nan; break;
        case 3: m.xyz[3 * i] = nan; break;
        case 4: m.xyz[3 * i + 1] = nan; break;
        case 5: m.xyz[3 * i + 2] = nan; break;
        case 6: m.xyz[3 * i] = inf; break;
        case 7: m.xyz[3 * i + 1] = -inf; break;
        case 8: m.xyz[3 * i + 2] = inf; break;
        case 9: m.op[i] = nan; break;
        case 10: m.op[i] = inf; break;
        case 11: m.op[i] = -inf; break;
        case 12: m.scale[3 * i + 1] = 1e18f; break;   // radius beyond INT_MAX: the whole grid
        default: return 0;
    }
    return 1;
}

static int render(const Model& m, int cull, int variant, int rows, std::vector<float>& img, std::vector<int>& radii) {
    gs2m_raster* r = nullptr;
    if (gs2m_raster_create(&r, 0)) return 1;
    int rc = gs2m_raster_set_option(r, GS2M_OPT_EXACT_TILE_CULL, cull) || gs2m_raster_set_option(r, GS2M_OPT_BLEND_VARIANT, variant) ||
             gs2m_raster_set_option(r, GS2M_OPT_TILE_ROWS, rows);
    float view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float zn = 0.01f, zf = 100.0f;
    float proj[16] = {2.0f * F / W, 0, 0, 0, 0, 2.0f * F / H, 0, 0, 0, 0, zf / (zf - zn), 1, 0, 0, -(zf * zn) / (zf - zn), 0};
    const float campos[3] = {0, 0, 0}, bg[3] = {0.1f, 0.2f, 0.3f};
    img.assign((size_t)3 * W * H, -1.0f);
    radii.assign((size_t)m.P(), -7);
    rc = rc || gs2m_rasterize_forward(r, m.P(), 0, 0, bg, W, H, m.xyz.data(), nullptr, m.col.data(), m.op.data(), m.scale.data(), 1.0f,
                                      m.rot.data(), nullptr, view, proj, campos, W / (2.0f * F), H / (2.0f * F), 0, img.data(),
                                      radii.data(), 0, nullptr);
    int64_t n = -1, required = 0;
    int overflow = 1;
    rc = rc || gs2m_raster_status(r, nullptr, 1, &n, &overflow, &required);
    if (rc) printf("error: %s\n", gs2m_last_error());
    CHECK(overflow == 0 && n >= 0);
    gs2m_raster_destroy(r);
    return rc;
}

int main() {
    Model clean;
    for (int j = 0; j < 5; ++j)
        for (int i = 0; i < 8; ++i) clean.add(4.0f + 8.0f * i, 2.0f + 7.0f * j, 2.0f + 0.01f * (float)(8 * j + i), 0.06f + 0.01f * (float)(i % 3), 0.3f + 0.1f * (float)(j % 5));
    Model bad = clean, huge = clean;
    const float at[2][2] = {{5.0f, 6.0f}, {40.0f, 24.0f}};   // tile (0, 0) and tile (2, 1): a splat of radius 5 stays inside each
    for (int p = 0; p < 2; ++p)
        for (int kind = 0; kind < 12; ++kind) {
            bad.add(at[p][0], at[p][1], 2.5f, 0.05f, 0.7f);
            CHECK(spoil(bad, kind));
        }
    for (int p = 0; p < 2; ++p) {
        huge.add(at[p][0], at[p][1], 2.5f, 0.05f, 0.7f);
        CHECK(spoil(huge, 12));
    }
    for (int cull = 0; cull <= 2; ++cull)
        for (int cfg = 0; cfg < 3; ++cfg) {
            const int variant = cfg == 0 ? 0 : 4, rows = cfg == 2 ? 2 : 1;
            std::vector<float> img0, img1, img2;
            std::vector<int> rad0, rad1, rad2;
            CHECK(render(clean, cull, variant, rows, img0, rad0) == 0);
            CHECK(render(bad, cull, variant, rows, img1, rad1) == 0);
            CHECK(render(huge, cull, variant, rows, img2, rad2) == 0);
            for (int i = 0; i < bad.P(); ++i) CHECK(rad1[i] >= 0 && (i >= clean.P() || rad1[i] == rad0[i]));
            for (int i = 0; i < clean.P(); ++i) CHECK(rad2[i] == rad0[i]);
            for (int i = clean.P(); i < huge.P(); ++i) CHECK(rad2[i] == 2147483647);
            int differing = 0;
            for (int c = 0; c < 3; ++c)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        const bool in_bad_tile = (x < 16 && y < 16) || (x >= 32 && x < 48 && y >= 16);
                        const size_t k = ((size_t)c * H + y) * W + x;
                        if (!in_bad_tile && memcmp(&img0[k], &img1[k], 4) != 0) ++differing;
                    }
            CHECK(differing == 0);
        }
    if (g_failed) return 1;
    printf("ok\n");
    return 0;
}
