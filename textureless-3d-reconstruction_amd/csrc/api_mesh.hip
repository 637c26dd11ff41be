// api_mesh.hip -- the mesh-in / mesh-out calls of the extern "C" surface (include/tl3d.h; the registration calls: api_register.hip,
// everything else: tl3d_api.hip): host code only, no call needs a grid.
// Each call carves its device scratch from the context's buffers (scratch_carve, api_host.h) by ONE size list at its top; the
// comment on the list names, array by array, the memset or kernel that writes it first -- nothing is read before.
#include <math.h>

#include <functional>
#include <vector>

#include "api_host.h"

using namespace tl3d;

extern "C" {

// the argument checks the calls share; none of them needs a device
static int cc_check_mesh(const uint32_t *tri, int64_t n_tri, int64_t n_vert, const char *tri_reason = "the component key needs") {
    REQUIRE(n_tri >= 0 && n_vert >= 0, TL3D_E_INVALID, "negative size (n_tri %lld, n_vert %lld)", (long long)n_tri, (long long)n_vert);
    REQUIRE(n_vert < (1ll << 31), TL3D_E_INVALID, "n_vert %lld: indices need fewer than 2^31 vertices", (long long)n_vert);
    REQUIRE(n_tri < (1ll << 32), TL3D_E_INVALID, "n_tri %lld: %s fewer than 2^32 triangles", (long long)n_tri, tri_reason);
    REQUIRE(n_tri == 0 || tri, TL3D_E_INVALID, "null triangle list");
    return TL3D_OK;
}

// What every size list ends with: the counts and the offsets per chunk of vertices / triangles (ChunkHalves), mio_chunks entries
// each, and the eight report words (tl3d_internal.h has their table)
static size_t mio_chunks(int64_t n_tri, int64_t n_vert) { return (size_t)chunks_of(n_vert) + (size_t)chunks_of(n_tri) + 2; }
constexpr size_t MIO_INFO_BYTES = 8 * sizeof(unsigned long long);

// The validation sequence of the calls that take one indexed mesh: the report words zeroed, the largest triangle index
// (cc_validate_kernel) into word 0, the caller's own validator (`second`, if it has one) into word 1, one wait, and the refusal of
// an index beyond n_vert.  *word1 = what `second` counted: the caller refuses it in its own words.  Nothing of the call indexes by
// a triangle, or takes a coordinate apart, before this has returned TL3D_OK.
static int mio_validate(tl3d_ctx *ctx, unsigned long long *info, const uint32_t *dtri, int64_t n_tri, int64_t n_vert,
                        const std::function<int()> &second = nullptr, unsigned long long *word1 = nullptr) {
    unsigned long long h[2] = {0, 0};
    TL3D_HIP(hipMemsetAsync(info, 0, MIO_INFO_BYTES, ctx->stream));
    int rc = launch_cc_validate(ctx->stream, dtri, n_tri, info);
    if (!rc && second) rc = second();
    if (rc) return rc;
    TL3D_HIP(hipMemcpyAsync(h, info, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    REQUIRE(n_tri == 0 || (int64_t)h[0] < n_vert, TL3D_E_INVALID, "triangle index %llu out of range [0, %lld)", h[0], (long long)n_vert);
    if (word1) *word1 = h[1];
    return TL3D_OK;
}

// What a call that takes an indexed mesh and returns one does with its arrays, whichever kernels run in between: the argument
// checks (their order, codes and texts are part of the interface), staging the three inputs, the capacity error, staging the
// three outputs.  The call's fourth output (one entry per input vertex) differs in size and stays with the call.
struct MeshIO {
    const float *xyz; const uint8_t *rgb; int64_t n_vert; const uint32_t *tri; int64_t n_tri;
    float *out_xyz; uint8_t *out_rgb; int64_t vert_cap; uint32_t *out_tri; int64_t tri_cap;
    const float *dxyz = nullptr; const uint8_t *drgb = nullptr; const uint32_t *dtri = nullptr;     // stage_in
    float *oxyz = nullptr; uint8_t *orgb = nullptr; uint32_t *otri = nullptr;                       // stage_out

    // sizes, capacities, and the call's count outputs (counts_given: none of them is null)
    int check_sizes(bool counts_given) const {
        const int rc = cc_check_mesh(tri, n_tri, n_vert);
        if (rc) return rc;
        REQUIRE(vert_cap >= 0 && tri_cap >= 0, TL3D_E_INVALID, "negative capacity");
        REQUIRE(counts_given, TL3D_E_INVALID, "null argument");
        return TL3D_OK;
    }
    // the arrays; extra_out: the call's fourth output, extra_bytes long
    int check_arrays(const void *extra_out, size_t extra_bytes) const {
        REQUIRE(n_vert == 0 || xyz, TL3D_E_INVALID, "null vertex list");
        REQUIRE((vert_cap == 0 || (out_xyz && (out_rgb || !rgb))) && (tri_cap == 0 || out_tri), TL3D_E_INVALID, "null output with a capacity");
        const void *ins[3] = {xyz, rgb, tri};
        const size_t in_b[3] = {(size_t)n_vert * 12, (size_t)n_vert * 3, (size_t)n_tri * 12};
        const void *outs[4] = {out_xyz, rgb ? out_rgb : nullptr, out_tri, extra_out};
        const size_t out_b[4] = {(size_t)vert_cap * 12, (size_t)vert_cap * 3, (size_t)tri_cap * 12, extra_bytes};
        for (int o = 0; o < 4; ++o)
            for (int i = 0; i < 3; ++i)
                REQUIRE(!ranges_overlap(outs[o], out_b[o], ins[i], in_b[i]), TL3D_E_INVALID, "an output aliases an input");
        return TL3D_OK;
    }
    int stage_in(Staging &st) {
        int rc = st.in(xyz, (size_t)n_vert * 12, &dxyz);
        if (!rc && rgb) rc = st.in(rgb, (size_t)n_vert * 3, &drgb);
        if (!rc && n_tri) rc = st.in(tri, (size_t)n_tri * 12, &dtri);
        return rc;
    }
    // tot: the vertices and triangles the result has
    int stage_out(Staging &st, const unsigned long long tot[2]) {
        if ((int64_t)tot[0] > vert_cap || (int64_t)tot[1] > tri_cap)
            return set_err(TL3D_E_CAPACITY, "need %llu vertices / %llu triangles, capacities %lld / %lld", tot[0], tot[1], (long long)vert_cap,
                           (long long)tri_cap);
        int rc = st.out(out_xyz, (size_t)tot[0] * 12, &oxyz);
        if (!rc && rgb) rc = st.out(out_rgb, (size_t)tot[0] * 3, &orgb);
        if (!rc) rc = st.out(out_tri, (size_t)tot[1] * 12, &otri);
        return rc;
    }
};

// ------------------------------------------------------------------------------------------- mesh components
// The scratch of both calls, 12 B per vertex and the chunks.  First writers:
//   parent, count   cc_init_kernel, every vertex (parent = union-find parents, then labels; count = triangles per label)
//   remap           cc_vert_write_kernel, the kept vertices; cc_tri_write_kernel reads it at a kept triangle's vertices only
//   counts          cc_vert_count_kernel / cc_tri_count_kernel, one word per chunk; the word behind a half's chunks is never used
//   offsets         scan_kernel, every chunk and the total behind them (no triangle: the total alone)
//   info            mio_validate's memset
struct CcScratch {
    unsigned *parent, *count, *remap, *counts;
    unsigned long long *offsets, *info;
};
static int cc_scratch(tl3d_ctx *ctx, int64_t n_tri, int64_t n_vert, CcScratch *sc) {
    const size_t vb = (size_t)n_vert * sizeof(unsigned), nch = mio_chunks(n_tri, n_vert);
    const size_t bytes[6] = {vb, vb, vb, nch * sizeof(unsigned), nch * sizeof(unsigned long long), MIO_INFO_BYTES};
    void *p[6];
    const int rc = scratch_carve(ctx, 0, bytes, 6, p, "mesh component scratch");
    if (rc) return rc;
    *sc = {(unsigned *)p[0], (unsigned *)p[1], (unsigned *)p[2], (unsigned *)p[3], (unsigned long long *)p[4], (unsigned long long *)p[5]};
    return TL3D_OK;
}

// The validation pass and, only when every index is below n_vert, the labelling: parent = labels, count = triangles per
// label, the report words: largest index, components, key of the largest component.  Waits for the stream once.
static int cc_label(tl3d_ctx *ctx, const CcScratch &sc, const uint32_t *dtri, int64_t n_tri, int64_t n_vert) {
    const int rc = mio_validate(ctx, sc.info, dtri, n_tri, n_vert);
    return rc ? rc : launch_cc_label(ctx->stream, dtri, n_tri, n_vert, sc.parent, sc.count, sc.info);
}

int tl3d_mesh_components(tl3d_ctx *ctx, const uint32_t *tri, int64_t n_tri, int64_t n_vert, uint32_t *label_out, uint32_t *tri_count_out,
                         int64_t *out_n_components) {
    int rc = cc_check_mesh(tri, n_tri, n_vert);
    if (rc) return rc;
    REQUIRE(out_n_components != nullptr && (n_vert == 0 || label_out), TL3D_E_INVALID, "null argument");
    const size_t tb = (size_t)n_tri * 12, vb = (size_t)n_vert * 4;
    REQUIRE(!ranges_overlap(label_out, vb, tri, tb) && !ranges_overlap(tri_count_out, vb, tri, tb) && !ranges_overlap(label_out, vb, tri_count_out, vb),
            TL3D_E_INVALID, "an output aliases an input (or the other output)");
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    *out_n_components = 0;
    if (n_vert == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    CcScratch sc;
    rc = cc_scratch(ctx, n_tri, n_vert, &sc);
    if (rc) return rc;
    Staging st(ctx);
    const uint32_t *dtri = nullptr;
    if (n_tri) rc = st.in(tri, tb, &dtri);
    if (rc) return rc;
    unsigned long long h[4] = {0, 0, 0, 0};
    rc = cc_label(ctx, sc, dtri, n_tri, n_vert);
    if (rc) return rc;
    TL3D_HIP(hipMemcpyAsync(label_out, sc.parent, vb, hipMemcpyDefault, ctx->stream));
    if (tri_count_out) TL3D_HIP(hipMemcpyAsync(tri_count_out, sc.count, vb, hipMemcpyDefault, ctx->stream));
    TL3D_HIP(hipMemcpyAsync(h, sc.info, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    *out_n_components = (int64_t)h[1];
    return TL3D_OK;
}

int tl3d_mesh_filter_components(tl3d_ctx *ctx, const float *xyz, const uint8_t *rgb, int64_t n_vert, const uint32_t *tri, int64_t n_tri,
                                int64_t min_triangles, int largest_only, float *out_xyz, uint8_t *out_rgb, int64_t vert_cap,
                                uint32_t *out_tri, int64_t tri_cap, uint8_t *keep_vert_out, int64_t *out_n_vert, int64_t *out_n_tri,
                                int64_t *out_n_components, int64_t *out_n_kept) {
    MeshIO m{xyz, rgb, n_vert, tri, n_tri, out_xyz, out_rgb, vert_cap, out_tri, tri_cap};
    int rc = m.check_sizes(out_n_vert && out_n_tri && out_n_components && out_n_kept);
    if (!rc) rc = m.check_arrays(keep_vert_out, (size_t)n_vert);
    if (rc) return rc;
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    *out_n_vert = *out_n_tri = *out_n_components = *out_n_kept = 0;
    if (n_vert == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    CcScratch sc;
    rc = cc_scratch(ctx, n_tri, n_vert, &sc);
    if (rc) return rc;
    Staging st(ctx);
    uint8_t *dkeep = nullptr;
    rc = m.stage_in(st);
    if (!rc && keep_vert_out) rc = st.out(keep_vert_out, (size_t)n_vert, &dkeep);
    if (rc) return rc;
    unsigned long long h[4] = {0, 0, 0, 0};
    rc = cc_label(ctx, sc, m.dtri, n_tri, n_vert);
    if (rc) return rc;
    const ChunkHalves ch(sc.counts, sc.offsets, chunks_of(n_vert), chunks_of(n_tri));
    rc = launch_cc_keep_count(ctx->stream, (long long)min_triangles, largest_only != 0, m.dtri, n_tri, n_vert, sc.parent, sc.count,
                              ch.counts[0], ch.counts[1], dkeep, sc.info);
    if (!rc) rc = ch.scan(ctx->stream, 0);
    if (!rc) rc = ch.scan(ctx->stream, 1);                                                   // (no triangle: the total is 0)
    unsigned long long tot[2] = {0, 0};
    if (!rc) rc = ch.totals(ctx->stream, tot, sc.info, h);
    if (rc) return rc;
    *out_n_vert = (int64_t)tot[0];
    *out_n_tri = (int64_t)tot[1];
    *out_n_components = (int64_t)h[1];
    *out_n_kept = (int64_t)h[3];
    rc = m.stage_out(st, tot);
    if (rc) return rc;
    rc = launch_cc_compact(ctx->stream, (long long)min_triangles, largest_only != 0, m.dtri, n_tri, n_vert, sc.parent, sc.count,
                           ch.offs[0], ch.offs[1], m.dxyz, m.drgb, m.oxyz, m.orgb, tot[0], m.otri, tot[1], sc.remap, sc.info);
    return st.finish(rc, true);
}

// ------------------------------------------------------------------------------------------- mesh simplification
// Both placements.  quadric: the three extra counts (placed, clamped, corners skipped), or nullptr for mean placement, which
// then launches, copies and waits exactly as it did before the quadric existed.
static int ms_simplify(tl3d_ctx *ctx, const float *xyz, const uint8_t *rgb, int64_t n_vert, const uint32_t *tri, int64_t n_tri, double cell,
                       const double origin[3], double reg, float *out_xyz, uint8_t *out_rgb, int64_t vert_cap, uint32_t *out_tri,
                       int64_t tri_cap, uint32_t *vert_map_out, int64_t *const counts[4], int64_t *const quadric[3]) {
    MeshIO m{xyz, rgb, n_vert, tri, n_tri, out_xyz, out_rgb, vert_cap, out_tri, tri_cap};
    int rc = m.check_sizes(counts[0] && counts[1] && counts[2] && counts[3] && (!quadric || (quadric[0] && quadric[1] && quadric[2])));
    if (rc) return rc;
    REQUIRE(std::isfinite(cell) && cell > 0.0, TL3D_E_INVALID, "cell size %g: must be finite and > 0", cell);
    const double o[3] = {origin ? origin[0] : 0.0, origin ? origin[1] : 0.0, origin ? origin[2] : 0.0};
    REQUIRE(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]), TL3D_E_INVALID, "origin (%g, %g, %g) is not finite", o[0], o[1], o[2]);
    REQUIRE(!quadric || (std::isfinite(reg) && reg > 0.0 && reg <= 1.0), TL3D_E_INVALID, "reg %g: must lie in (0, 1]", reg);
    rc = m.check_arrays(vert_map_out, (size_t)n_vert * 4);
    if (rc) return rc;
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    for (int k = 0; k < 4; ++k) *counts[k] = 0;
    for (int k = 0; quadric && k < 3; ++k) *quadric[k] = 0;
    if (n_vert == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    // The scratch.  First writers:
    //   keys, leader    memset 0xFF below (the vertex table: a cell key per slot and, beside it, the cluster's leader)
    //   slot            ms_insert_kernel, every vertex (its slot in the table)
    //   vmap            ms_leader_write_kernel (the leaders), then ms_accumulate_kernel (the members): the cluster number
    //   acc, qacc       memset 0 below (seven 64-bit sums per cluster; quadric only: nine 128-bit sums as (lo, hi))
    //   ttab            memset 0xFF below (the triangle table, one index per slot)
    //   flag            ms_tri_count_kernel, every triangle (its class byte)
    //   counts          ms_leader_count_kernel / ms_tri_count_kernel, one word per chunk; offsets: scan_kernel
    //   info            mio_validate's memset
    struct { unsigned long long *keys; unsigned *leader, *slot, *vmap; unsigned long long *acc, *qacc; unsigned *ttab; uint8_t *flag;
             unsigned *counts; unsigned long long *offsets, *info; } sc;
    const size_t nv = (size_t)n_vert, vslots = kt_slots(nv), tslots = kt_slots((size_t)n_tri), nch = mio_chunks(n_tri, n_vert);
    const size_t bytes[11] = {vslots * sizeof(unsigned long long), vslots * sizeof(unsigned), nv * sizeof(unsigned), nv * sizeof(unsigned),
                              7 * nv * sizeof(unsigned long long), quadric ? 18 * nv * sizeof(unsigned long long) : 0,
                              n_tri ? tslots * sizeof(unsigned) : 0, (size_t)n_tri, nch * sizeof(unsigned), nch * sizeof(unsigned long long),
                              MIO_INFO_BYTES};
    void *p[11];
    rc = scratch_carve(ctx, 0, bytes, 11, p, "mesh simplification scratch");
    if (rc) return rc;
    sc = {(unsigned long long *)p[0], (unsigned *)p[1], (unsigned *)p[2], (unsigned *)p[3], (unsigned long long *)p[4],
          quadric ? (unsigned long long *)p[5] : nullptr, (unsigned *)p[6], (uint8_t *)p[7], (unsigned *)p[8], (unsigned long long *)p[9],
          (unsigned long long *)p[10]};
    rc = kt_reserve(ctx, sc.keys, vslots);
    if (rc) return rc;
    Staging st(ctx);
    rc = m.stage_in(st);
    if (rc) return rc;
    // the validation passes: nothing is indexed, and no cell is computed for a table, before the host has seen their words
    unsigned long long h[4] = {0, 0, 0, 0}, hq[3] = {0, 0, 0};
    rc = mio_validate(ctx, sc.info, m.dtri, n_tri, n_vert, [&] { return launch_ms_validate(ctx->stream, cell, o, m.dxyz, n_vert, sc.info); }, &h[1]);
    if (rc) return rc;
    REQUIRE(h[1] == 0, TL3D_E_INVALID, "%llu vertices are not finite or lie 2^20 cells or more from the origin", h[1]);
    const ChunkHalves ch(sc.counts, sc.offsets, chunks_of(n_vert), chunks_of(n_tri));
    unsigned long long *qacc = sc.qacc;                     // (nullptr: mean placement)
    TL3D_HIP(hipMemsetAsync(sc.leader, 0xFF, vslots * sizeof(unsigned), ctx->stream));
    TL3D_HIP(hipMemsetAsync(sc.acc, 0, 7 * nv * sizeof(unsigned long long), ctx->stream));
    if (qacc) TL3D_HIP(hipMemsetAsync(qacc, 0, 18 * nv * sizeof(unsigned long long), ctx->stream));
    if (n_tri) TL3D_HIP(hipMemsetAsync(sc.ttab, 0xFF, tslots * sizeof(unsigned), ctx->stream));
    rc = launch_ms_cluster(ctx->stream, cell, o, m.dxyz, m.drgb, n_vert, sc.keys, sc.leader, vslots, sc.slot, sc.vmap, sc.acc, ch.counts[0],
                           ch.offs[0]);
    if (!rc && qacc) rc = launch_ms_quadrics(ctx->stream, cell, o, m.dxyz, m.dtri, n_tri, sc.vmap, qacc, sc.info);
    if (!rc) rc = launch_ms_triangles(ctx->stream, m.dtri, n_tri, sc.vmap, sc.ttab, tslots, sc.flag, ch.counts[1], ch.offs[1], sc.info);
    unsigned long long tot[2] = {0, 0};
    if (!rc) rc = ch.totals(ctx->stream, tot, sc.info, h);
    if (rc) return rc;
    *counts[0] = (int64_t)tot[0];
    *counts[1] = (int64_t)tot[1];
    *counts[2] = (int64_t)h[2];
    *counts[3] = (int64_t)h[3];
    rc = m.stage_out(st, tot);
    if (rc == TL3D_E_CAPACITY && quadric) {
        // the solve counts what it places and clamps: run it without outputs, so that the refusal reports all seven counts
        int rq = launch_ms_write(ctx->stream, cell, o, m.dxyz, false, n_vert, sc.slot, sc.leader, sc.vmap, sc.acc, nullptr, nullptr, 0, m.dtri, n_tri,
                                 sc.flag, ch.offs[1], nullptr, 0, qacc, reg, sc.info);
        if (rq) return rq;
        TL3D_HIP(hipMemcpyAsync(hq, sc.info + 4, sizeof(hq), hipMemcpyDeviceToHost, ctx->stream));
        TL3D_HIP(hipStreamSynchronize(ctx->stream));
        *quadric[0] = (int64_t)hq[1]; *quadric[1] = (int64_t)hq[2]; *quadric[2] = (int64_t)hq[0];
    }
    if (rc) return rc;
    rc = launch_ms_write(ctx->stream, cell, o, m.dxyz, rgb != nullptr, n_vert, sc.slot, sc.leader, sc.vmap, sc.acc, m.oxyz, m.orgb, tot[0], m.dtri,
                         n_tri, sc.flag, ch.offs[1], m.otri, tot[1], qacc, reg, sc.info);
    if (!rc && vert_map_out) TL3D_HIP(hipMemcpyAsync(vert_map_out, sc.vmap, (size_t)n_vert * 4, hipMemcpyDefault, ctx->stream));
    if (!rc && quadric) TL3D_HIP(hipMemcpyAsync(hq, sc.info + 4, sizeof(hq), hipMemcpyDeviceToHost, ctx->stream));
    rc = st.finish(rc, true);
    if (!rc && quadric) { *quadric[0] = (int64_t)hq[1]; *quadric[1] = (int64_t)hq[2]; *quadric[2] = (int64_t)hq[0]; }
    return rc;
}

int tl3d_mesh_simplify_clusters(tl3d_ctx *ctx, const float *xyz, const uint8_t *rgb, int64_t n_vert, const uint32_t *tri, int64_t n_tri,
                                double cell, const double origin[3], float *out_xyz, uint8_t *out_rgb, int64_t vert_cap,
                                uint32_t *out_tri, int64_t tri_cap, uint32_t *vert_map_out, int64_t *out_n_vert, int64_t *out_n_tri,
                                int64_t *out_n_degenerate, int64_t *out_n_duplicate) {
    int64_t *const counts[4] = {out_n_vert, out_n_tri, out_n_degenerate, out_n_duplicate};
    return ms_simplify(ctx, xyz, rgb, n_vert, tri, n_tri, cell, origin, 0.0, out_xyz, out_rgb, vert_cap, out_tri, tri_cap, vert_map_out, counts,
                       nullptr);
}

int tl3d_mesh_simplify_quadric(tl3d_ctx *ctx, const float *xyz, const uint8_t *rgb, int64_t n_vert, const uint32_t *tri, int64_t n_tri,
                               double cell, const double origin[3], double reg, float *out_xyz, uint8_t *out_rgb, int64_t vert_cap,
                               uint32_t *out_tri, int64_t tri_cap, uint32_t *vert_map_out, int64_t *out_n_vert, int64_t *out_n_tri,
                               int64_t *out_n_degenerate, int64_t *out_n_duplicate, int64_t *out_n_quadric, int64_t *out_n_clamped,
                               int64_t *out_n_skipped) {
    int64_t *const counts[4] = {out_n_vert, out_n_tri, out_n_degenerate, out_n_duplicate};
    int64_t *const quadric[3] = {out_n_quadric, out_n_clamped, out_n_skipped};
    return ms_simplify(ctx, xyz, rgb, n_vert, tri, n_tri, cell, origin, reg, out_xyz, out_rgb, vert_cap, out_tri, tri_cap, vert_map_out, counts,
                       quadric);
}

// ------------------------------------------------------------------------------------------- mesh smoothing, vertex normals
// the two validation passes and the host's look at their words: nothing is indexed, and no coordinate is quantised, before it
static int adj_validate(tl3d_ctx *ctx, unsigned long long *info, const float *dxyz, int64_t n_vert, const uint32_t *dtri, int64_t n_tri) {
    unsigned long long bad = 0;
    const int rc = mio_validate(ctx, info, dtri, n_tri, n_vert, [&] { return launch_msm_validate(ctx->stream, dxyz, n_vert, info); }, &bad);
    if (rc) return rc;
    REQUIRE(bad == 0, TL3D_E_INVALID, "%llu vertices are not finite or lie beyond 2^20 m", bad);
    return TL3D_OK;
}

int tl3d_mesh_smooth_taubin(tl3d_ctx *ctx, const float *xyz, int64_t n_vert, const uint32_t *tri, int64_t n_tri, int iterations, double lambda,
                            double mu, float *out_xyz, uint32_t *valence_out, int64_t *out_n_edges) {
    const char *what = "mesh smoothing scratch";
    int rc = cc_check_mesh(tri, n_tri, n_vert, "the triangle and corner counts need");
    if (rc) return rc;
    REQUIRE(out_n_edges != nullptr && (n_vert == 0 || (xyz && out_xyz)), TL3D_E_INVALID, "null argument");
    REQUIRE(iterations >= 0 && iterations <= 1000, TL3D_E_INVALID, "iterations %d out of range [0, 1000]", iterations);
    REQUIRE(lambda > 0.0 && lambda <= 1.0, TL3D_E_INVALID, "lambda %g out of range (0, 1]", lambda);             // (false for NaN)
    REQUIRE(mu >= -2.0 && mu <= 0.0, TL3D_E_INVALID, "mu %g out of range [-2, 0]", mu);
    const size_t xb = (size_t)n_vert * 12, tb = (size_t)n_tri * 12, vb = (size_t)n_vert * 4;
    REQUIRE(!ranges_overlap(out_xyz, xb, xyz, xb) && !ranges_overlap(out_xyz, xb, tri, tb) && !ranges_overlap(valence_out, vb, xyz, xb) &&
                !ranges_overlap(valence_out, vb, tri, tb) && !ranges_overlap(valence_out, vb, out_xyz, xb),
            TL3D_E_INVALID, "an output aliases an input (or the other output)");
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    *out_n_edges = 0;
    if (n_vert == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    // The scratch.  First writers:
    //   cnt             memset 0 below (the valence: msm_edge_insert_kernel adds to it)
    //   cursor, row     msm_row_write_kernel, every vertex (fill cursor 0; the 64-bit offset of the vertex's row)
    //   ccounts, coffs  msm_row_count_kernel, one 64-bit sum per chunk; scan_kernel, every chunk and the total
    //   keys            memset 0xFF below (the edge table: a triangle brings at most three keys; no word beside them)
    //   xyz2            msm_step_kernel, every vertex, by the first step (the second position buffer of the steps)
    //   counts, offsets never used (carved like every mesh call's)
    //   info            mio_validate's memset
    //   nbr (stage 1)   msm_edge_fill_kernel, each of the 2 E entries once (the neighbour rows)
    struct { unsigned *cnt, *cursor; unsigned long long *row, *ccounts, *coffs, *keys; float *xyz2; unsigned *counts;
             unsigned long long *offsets, *info; unsigned *nbr; } sc;
    const size_t slots = kt_slots(3 * (size_t)n_tri), rch = (size_t)chunks_of(n_vert) + 1, nch = mio_chunks(n_tri, n_vert);
    const size_t bytes[10] = {vb, vb, (size_t)n_vert * sizeof(unsigned long long), rch * sizeof(unsigned long long),
                              rch * sizeof(unsigned long long), n_tri ? slots * sizeof(unsigned long long) : 0,
                              n_tri && iterations ? xb : 0, nch * sizeof(unsigned), nch * sizeof(unsigned long long), MIO_INFO_BYTES};
    void *p[10];
    rc = scratch_carve(ctx, 0, bytes, 10, p, what);
    if (rc) return rc;
    sc = {(unsigned *)p[0], (unsigned *)p[1], (unsigned long long *)p[2], (unsigned long long *)p[3], (unsigned long long *)p[4],
          (unsigned long long *)p[5], (float *)p[6], (unsigned *)p[7], (unsigned long long *)p[8], (unsigned long long *)p[9], nullptr};
    if (n_tri) rc = kt_reserve(ctx, sc.keys, slots);
    if (rc) return rc;
    Staging st(ctx);
    const float *dxyz = nullptr;
    const uint32_t *dtri = nullptr;
    float *oxyz = nullptr;
    uint32_t *oval = nullptr;
    rc = st.in(xyz, xb, &dxyz);
    if (!rc && n_tri) rc = st.in(tri, tb, &dtri);
    if (!rc) rc = st.out(out_xyz, xb, &oxyz);
    if (!rc && valence_out) rc = st.out(valence_out, vb, &oval);
    if (!rc) rc = adj_validate(ctx, sc.info, dxyz, n_vert, dtri, n_tri);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    TL3D_HIP(hipMemsetAsync(sc.cnt, 0, vb, s));
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    if (n_tri) {
        rc = launch_msm_edges(s, dtri, n_tri, sc.keys, slots, sc.cnt, sc.info);
        if (rc) return rc;
        TL3D_HIP(hipMemcpyAsync(h, sc.info, sizeof(h), hipMemcpyDeviceToHost, s));
        TL3D_HIP(hipStreamSynchronize(s));
    }
    *out_n_edges = (int64_t)h[2];
    if (oval) TL3D_HIP(hipMemcpyAsync(oval, sc.cnt, vb, hipMemcpyDeviceToDevice, s));
    if (h[2] == 0 || iterations == 0) {                    // nothing moves
        TL3D_HIP(hipMemcpyAsync(oxyz, dxyz, xb, hipMemcpyDeviceToDevice, s));
        return st.finish(TL3D_OK, true);
    }
    const size_t nbr_bytes = 2 * (size_t)h[2] * sizeof(unsigned);          // exact: the host has just seen the edge count
    rc = scratch_carve(ctx, 1, &nbr_bytes, 1, (void **)&sc.nbr, what);
    if (!rc) rc = launch_msm_rows(s, sc.cnt, n_vert, sc.ccounts, sc.coffs, sc.row, sc.cursor);
    if (!rc) rc = launch_msm_edge_fill(s, sc.keys, slots, sc.cnt, sc.row, sc.cursor, sc.nbr);
    // 2 * iterations steps between the scratch buffer and the output: in -> scratch -> out -> scratch -> out ...
    const float *src = dxyz;
    for (int i = 0; i < 2 * iterations && !rc; ++i) {
        float *dst = (i & 1) ? oxyz : sc.xyz2;
        // the divergence flag: step i reports through word 3 + (i & 1) and reads the word of the step before it (both zero at first)
        rc = launch_msm_step(s, src, dst, n_vert, sc.cnt, sc.row, sc.nbr, (i & 1) ? mu : lambda, sc.info + 4 - (i & 1), sc.info + 3 + (i & 1));
        src = dst;
    }
    if (rc) return rc;
    TL3D_HIP(hipMemcpyAsync(h, sc.info, sizeof(h), hipMemcpyDeviceToHost, s));
    rc = st.finish(TL3D_OK, true);
    if (rc) return rc;
    REQUIRE((h[3] | h[4]) == 0, TL3D_E_INVALID,
            "smoothing diverged: a step gave a coordinate that is not finite or lies beyond 2^20 m (lambda %g, mu %g)", lambda, mu);
    return TL3D_OK;
}

int tl3d_mesh_vertex_normals(tl3d_ctx *ctx, const float *xyz, int64_t n_vert, const uint32_t *tri, int64_t n_tri, float *out_normal,
                             int64_t *out_n_zero) {
    int rc = cc_check_mesh(tri, n_tri, n_vert, "the triangle ids of the rows need");
    if (rc) return rc;
    REQUIRE(out_n_zero != nullptr && (n_vert == 0 || (xyz && out_normal)), TL3D_E_INVALID, "null argument");
    const size_t xb = (size_t)n_vert * 12, tb = (size_t)n_tri * 12, vb = (size_t)n_vert * 4;
    REQUIRE(!ranges_overlap(out_normal, xb, xyz, xb) && !ranges_overlap(out_normal, xb, tri, tb), TL3D_E_INVALID, "an output aliases an input");
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    *out_n_zero = 0;
    if (n_vert == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    // The scratch.  First writers:
    //   cnt             memset 0 below (incident corners: msm_corner_count_kernel adds to it)
    //   cursor, row, ccounts, coffs   as for smoothing (launch_msm_rows inside launch_msm_corners)
    //   inc             msm_corner_fill_kernel, each of the 3 n_tri entries once (the triangle ids of the rows)
    //   counts, offsets never used (carved like every mesh call's)
    //   info            mio_validate's memset
    struct { unsigned *cnt, *cursor; unsigned long long *row, *ccounts, *coffs; unsigned *inc, *counts; unsigned long long *offsets, *info; } sc;
    const size_t rch = (size_t)chunks_of(n_vert) + 1, nch = mio_chunks(n_tri, n_vert);
    const size_t bytes[9] = {vb, vb, (size_t)n_vert * sizeof(unsigned long long), rch * sizeof(unsigned long long),
                             rch * sizeof(unsigned long long), 3 * (size_t)n_tri * sizeof(unsigned), nch * sizeof(unsigned),
                             nch * sizeof(unsigned long long), MIO_INFO_BYTES};
    void *p[9];
    rc = scratch_carve(ctx, 0, bytes, 9, p, "mesh normal scratch");
    if (rc) return rc;
    sc = {(unsigned *)p[0], (unsigned *)p[1], (unsigned long long *)p[2], (unsigned long long *)p[3], (unsigned long long *)p[4],
          (unsigned *)p[5], (unsigned *)p[6], (unsigned long long *)p[7], (unsigned long long *)p[8]};
    Staging st(ctx);
    const float *dxyz = nullptr;
    const uint32_t *dtri = nullptr;
    float *onrm = nullptr;
    rc = st.in(xyz, xb, &dxyz);
    if (!rc && n_tri) rc = st.in(tri, tb, &dtri);
    if (!rc) rc = st.out(out_normal, xb, &onrm);
    if (!rc) rc = adj_validate(ctx, sc.info, dxyz, n_vert, dtri, n_tri);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    if (n_tri == 0) {
        TL3D_HIP(hipMemsetAsync(onrm, 0, xb, s));
        *out_n_zero = n_vert;
        return st.finish(TL3D_OK, true);
    }
    TL3D_HIP(hipMemsetAsync(sc.cnt, 0, vb, s));
    rc = launch_msm_corners(s, dtri, n_tri, n_vert, sc.cnt, sc.ccounts, sc.coffs, sc.row, sc.cursor, sc.inc);
    if (!rc) rc = launch_msm_normals(s, dxyz, dtri, n_vert, sc.cnt, sc.row, sc.inc, onrm, sc.info);
    if (rc) return rc;
    unsigned long long h[4] = {0, 0, 0, 0};
    TL3D_HIP(hipMemcpyAsync(h, sc.info, sizeof(h), hipMemcpyDeviceToHost, s));
    rc = st.finish(TL3D_OK, true);
    if (rc) return rc;
    *out_n_zero = (int64_t)h[3];
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- mesh weld
// Waits for the stream three times, however many parts there are: behind the validation pass, behind the scan (the number kept sizes
// the table and is compared with the capacity), and at the end.
int tl3d_mesh_weld_keyed(tl3d_ctx *ctx, const tl3d_mesh_part *parts, int n_parts, const int64_t lattice_dims[3], float *out_xyz,
                         uint8_t *out_rgb, int64_t *out_key, int64_t vert_cap, uint32_t *out_tri, int64_t tri_cap, int64_t *out_n_vert,
                         int64_t *out_n_tri, int64_t *out_n_twice, int64_t *out_n_unowned) {
    const char *what = "mesh weld scratch";
    REQUIRE(lattice_dims && out_n_vert && out_n_tri && out_n_twice && out_n_unowned && (n_parts <= 0 || parts), TL3D_E_INVALID, "null argument");
    REQUIRE(n_parts >= 0, TL3D_E_INVALID, "n_parts %d is negative", n_parts);
    REQUIRE(vert_cap >= 0 && tri_cap >= 0, TL3D_E_INVALID, "negative capacity");
    int64_t nv_tot = 0, nt_tot = 0;
    int with_rgb = 0, with_verts = 0;
    for (int p = 0; p < n_parts; ++p) {
        const tl3d_mesh_part &m = parts[p];
        REQUIRE(m.n_vert >= 0 && m.n_tri >= 0, TL3D_E_INVALID, "part %d: negative size (n_vert %lld, n_tri %lld)", p, (long long)m.n_vert,
                (long long)m.n_tri);
        REQUIRE(m.n_vert < (1ll << 31), TL3D_E_INVALID, "part %d: n_vert %lld: indices need fewer than 2^31 vertices", p, (long long)m.n_vert);
        REQUIRE(m.n_tri < (1ll << 32), TL3D_E_INVALID, "part %d: n_tri %lld: needs fewer than 2^32 triangles", p, (long long)m.n_tri);
        REQUIRE((m.n_vert == 0 || (m.xyz_hd && m.key_hd)) && (m.n_tri == 0 || m.tri_hd), TL3D_E_INVALID, "null argument (part %d)", p);
        nv_tot += m.n_vert;
        nt_tot += m.n_tri;
        with_verts += m.n_vert > 0;
        with_rgb += m.n_vert > 0 && m.rgb_hd;
    }
    REQUIRE(nt_tot < (1ll << 32), TL3D_E_INVALID, "%lld triangles in all: the welded mesh needs fewer than 2^32 triangles", (long long)nt_tot);
    REQUIRE(nv_tot < (1ll << 40), TL3D_E_INVALID, "%lld vertices in all: the weld needs fewer than 2^40 input vertices", (long long)nv_tot);
    unsigned __int128 nlat = 1;
    for (int a = 0; a < 3; ++a) {
        REQUIRE(lattice_dims[a] > 0, TL3D_E_INVALID, "lattice of %lld voxels on axis %d", (long long)lattice_dims[a], a);
        nlat *= (unsigned __int128)lattice_dims[a];
        REQUIRE(nlat < ((unsigned __int128)1 << 61), TL3D_E_INVALID, "lattice of 2^61 voxels or more: mesh keys would overflow");
    }
    for (int p = 0; p < n_parts; ++p)
        for (int a = 0; a < 3; ++a)
            REQUIRE(parts[p].core_lo[a] >= 0 && parts[p].core_lo[a] <= parts[p].core_hi[a] && parts[p].core_hi[a] <= lattice_dims[a], TL3D_E_INVALID,
                    "part %d: core [%lld, %lld) on axis %d must be a range within the lattice's %lld voxels", p, (long long)parts[p].core_lo[a],
                    (long long)parts[p].core_hi[a], a, (long long)lattice_dims[a]);
    REQUIRE(with_rgb == 0 || with_rgb == with_verts, TL3D_E_INVALID, "rgb given in some parts only (%d of %d)", with_rgb, with_verts);
    const bool rgb = with_rgb > 0;
    REQUIRE((vert_cap == 0 || (out_xyz && (out_rgb || !rgb))) && (tri_cap == 0 || out_tri), TL3D_E_INVALID, "null output with a capacity");
    {
        const void *outs[4] = {out_xyz, rgb ? out_rgb : nullptr, out_key, out_tri};
        const size_t out_b[4] = {(size_t)vert_cap * 12, (size_t)vert_cap * 3, (size_t)vert_cap * 8, (size_t)tri_cap * 12};
        for (int p = 0; p < n_parts; ++p) {
            const tl3d_mesh_part &m = parts[p];
            const void *ins[4] = {m.xyz_hd, m.rgb_hd, m.key_hd, m.tri_hd};
            const size_t in_b[4] = {(size_t)m.n_vert * 12, (size_t)m.n_vert * 3, (size_t)m.n_vert * 8, (size_t)m.n_tri * 12};
            for (int o = 0; o < 4; ++o)
                for (int i = 0; i < 4; ++i)
                    REQUIRE(!ranges_overlap(outs[o], out_b[o], ins[i], in_b[i]), TL3D_E_INVALID, "an output aliases an input (part %d)", p);
        }
    }
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    *out_n_vert = *out_n_tri = *out_n_twice = *out_n_unowned = 0;
    if (n_parts == 0 || nv_tot == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    // The scratch.  First writers:
    //   counts, offsets wm_own_count_kernel, one word per chunk of input vertices; scan_kernel, every chunk and the total
    //   vmap            wm_own_write_kernel, every input vertex (its output index, or NONE)
    //   parts           the descriptor upload below
    //   info            memset 0 below
    //   keys (stage 1)  memset 0xFF below (the key table: a key per slot)
    //   vals (stage 1)  wm_own_write_kernel beside each key it wins (the kept vertex's output index); wm_resolve_kernel reads
    //                   the word of a key it has found, nothing else
    struct { unsigned *counts; unsigned long long *offsets; unsigned *vmap; WeldPart *parts; unsigned long long *info, *keys; unsigned *vals; } sc;
    const size_t nch = mio_chunks(0, nv_tot);
    const size_t bytes[5] = {nch * sizeof(unsigned), nch * sizeof(unsigned long long), (size_t)nv_tot * sizeof(unsigned),
                             ((size_t)n_parts + 1) * sizeof(WeldPart), MIO_INFO_BYTES};
    void *cv[5];
    int rc = scratch_carve(ctx, 0, bytes, 5, cv, what);
    if (rc) return rc;
    sc = {(unsigned *)cv[0], (unsigned long long *)cv[1], (unsigned *)cv[2], (WeldPart *)cv[3], (unsigned long long *)cv[4], nullptr, nullptr};
    hipStream_t s = ctx->stream;
    // the inputs: a device array is read where it is; the host arrays of a kind are uploaded into one temporary, part behind part
    // (desc is declared in front of st: it is uploaded asynchronously, and st's destructor is what waits for the stream on every
    // way out.  st holds at most 4 input temporaries and 4 output temporaries: exactly Staging's MAX.)
    std::vector<WeldPart> desc((size_t)n_parts + 1);
    Staging st(ctx);
    {
        const size_t unit[4] = {12, 3, 8, 12};
        size_t host_b[4] = {0, 0, 0, 0};
        std::vector<uint8_t> on_host((size_t)n_parts * 4, 0);
        for (int p = 0; p < n_parts; ++p) {
            const tl3d_mesh_part &m = parts[p];
            const void *ins[4] = {m.xyz_hd, rgb ? m.rgb_hd : nullptr, m.key_hd, m.tri_hd};
            const size_t in_b[4] = {(size_t)m.n_vert * 12, (size_t)m.n_vert * 3, (size_t)m.n_vert * 8, (size_t)m.n_tri * 12};
            for (int k = 0; k < 4; ++k)
                if (ins[k] && in_b[k] && !is_device_ptr(ins[k])) {
                    on_host[(size_t)p * 4 + k] = 1;
                    host_b[k] += in_b[k];
                }
        }
        uint8_t *slab[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int k = 0; k < 4 && !rc; ++k)
            if (host_b[k]) rc = st.scratch(host_b[k], &slab[k]);
        if (rc) return rc;
        size_t used[4] = {0, 0, 0, 0};
        unsigned long long v0 = 0, t0 = 0;
        for (int p = 0; p < n_parts; ++p) {
            const tl3d_mesh_part &m = parts[p];
            const void *ins[4] = {m.xyz_hd, rgb ? m.rgb_hd : nullptr, m.key_hd, m.tri_hd};
            const size_t cnt[4] = {(size_t)m.n_vert, (size_t)m.n_vert, (size_t)m.n_vert, (size_t)m.n_tri};
            for (int k = 0; k < 4; ++k)
                if (on_host[(size_t)p * 4 + k]) {
                    void *d = slab[k] + used[k];
                    TL3D_HIP(hipMemcpyAsync(d, ins[k], cnt[k] * unit[k], hipMemcpyHostToDevice, s));
                    used[k] += cnt[k] * unit[k];
                    ins[k] = d;
                }
            WeldPart &w = desc[(size_t)p];
            w.xyz = (const float *)ins[0];
            w.rgb = (const uint8_t *)ins[1];
            w.key = (const long long *)ins[2];
            w.tri = (const unsigned *)ins[3];
            w.v0 = v0;
            w.t0 = t0;
            for (int a = 0; a < 3; ++a) {
                w.lo[a] = (long long)m.core_lo[a];
                w.hi[a] = (long long)m.core_hi[a];
            }
            v0 += (unsigned long long)m.n_vert;
            t0 += (unsigned long long)m.n_tri;
        }
        memset(&desc[(size_t)n_parts], 0, sizeof(WeldPart));
        desc[(size_t)n_parts].v0 = v0;
        desc[(size_t)n_parts].t0 = t0;
        TL3D_HIP(hipMemcpyAsync(sc.parts, desc.data(), desc.size() * sizeof(WeldPart), hipMemcpyHostToDevice, s));
    }
    const long long lat[3] = {(long long)lattice_dims[0], (long long)lattice_dims[1], (long long)lattice_dims[2]};
    const unsigned long long nv = (unsigned long long)nv_tot, nt = (unsigned long long)nt_tot;
    // the validation pass: nothing is indexed, and no key is taken apart, before the host has seen its words
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    TL3D_HIP(hipMemsetAsync(sc.info, 0, MIO_INFO_BYTES, s));
    rc = launch_wm_validate(s, sc.parts, n_parts, nv, nt, 3ull * (unsigned long long)nlat, sc.info);
    if (rc) return rc;
    TL3D_HIP(hipMemcpyAsync(h, sc.info, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));
    REQUIRE(h[0] == 0, TL3D_E_INVALID, "%llu triangle indices out of range (the largest: %llu in part %llu, which has %lld vertices)", h[0],
            h[2] & 0xffffffffull, h[2] >> 32, (long long)parts[h[2] >> 32].n_vert);
    REQUIRE(h[1] == 0, TL3D_E_INVALID, "%llu keys outside [0, 3 * %llu lattice voxels)", h[1], (unsigned long long)nlat);
    // the kept vertices
    const int chunks = chunks_of(nv);
    unsigned long long kept = 0;
    rc = launch_wm_own_count(s, sc.parts, n_parts, nv, lat, sc.counts, sc.offsets);
    if (rc) return rc;
    TL3D_HIP(hipMemcpyAsync(&kept, sc.offsets + chunks, sizeof(kept), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));
    *out_n_vert = (int64_t)kept;
    *out_n_tri = nt_tot;
    REQUIRE(kept < (1ull << 31), TL3D_E_CAPACITY, "%llu kept vertices: triangle indices need fewer than 2^31", kept);
    if ((int64_t)kept > vert_cap || nt_tot > tri_cap)
        return set_err(TL3D_E_CAPACITY, "need %llu vertices / %lld triangles, capacities %lld / %lld", kept, (long long)nt_tot, (long long)vert_cap,
                       (long long)tri_cap);
    float *oxyz = nullptr;
    uint8_t *orgb = nullptr;
    int64_t *okey = nullptr;
    uint32_t *otri = nullptr;
    rc = st.out(out_xyz, (size_t)kept * 12, &oxyz);
    if (!rc && rgb) rc = st.out(out_rgb, (size_t)kept * 3, &orgb);
    if (!rc && out_key) rc = st.out(out_key, (size_t)kept * 8, &okey);
    if (!rc) rc = st.out(out_tri, (size_t)nt * 12, &otri);
    const size_t slots = kt_slots((size_t)kept);           // the key table: a key per slot and, in the word beside it, the kept vertex's output index
    const size_t kt_bytes[2] = {slots * sizeof(unsigned long long), slots * sizeof(unsigned)};
    void *kt[2] = {nullptr, nullptr};
    if (!rc) rc = scratch_carve(ctx, 1, kt_bytes, 2, kt, what);
    sc.keys = (unsigned long long *)kt[0];
    sc.vals = (unsigned *)kt[1];
    if (!rc) rc = kt_reserve(ctx, sc.keys, slots);
    if (rc) return rc;
    rc = launch_wm_own_write(s, sc.parts, n_parts, nv, lat, sc.offsets, oxyz, orgb, (long long *)okey, kept, sc.vmap, sc.keys, sc.vals, slots,
                             sc.info);
    if (!rc) rc = launch_wm_resolve(s, sc.parts, n_parts, nt, sc.vmap, sc.keys, sc.vals, slots, otri, sc.info);
    if (rc) return rc;
    TL3D_HIP(hipMemcpyAsync(h, sc.info, sizeof(h), hipMemcpyDeviceToHost, s));
    rc = st.finish(TL3D_OK, true);
    if (rc) return rc;
    *out_n_twice = (int64_t)h[3];
    *out_n_unowned = (int64_t)h[4];
    REQUIRE(h[3] == 0, TL3D_E_INVALID, "a vertex is owned by two block cores (%llu kept vertices repeat a key: the cores overlap)", h[3]);
    REQUIRE(h[4] == 0, TL3D_E_INVALID, "a triangle references a vertex no block core owns (%llu corners: a halo is missing)", h[4]);
    return TL3D_OK;
}

}  // extern "C"
