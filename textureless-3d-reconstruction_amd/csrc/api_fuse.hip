// api_fuse.hip -- the fusion calls of the extern "C" surface (tl3d_integrate, tl3d_fuse_frames, tl3d_accumulate_centroid,
// tl3d_accumulate_points, tl3d_count_bricks, the cache read-outs) and the one path every TSDF prep chain takes to the device:
// the per-slot caches' look-ups, the ordering rule around them (ChainOrder), issue_prep_chain, flush_updates.  Host code only.
#include <math.h>

#include <new>

#include "api_host.h"

using namespace tl3d;

static PoseF make_pose_f(const double R[9], const double t[3]) {
    PoseF p;
    for (int i = 0; i < 9; ++i) p.r[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) p.t[i] = (float)t[i];
    return p;
}

static Frustum make_frustum(const Cam &c) {
    // inside: aL <= x/z <= aR, aT <= y/z <= aB, widened by one pixel on every side
    const double aL = (-1.5 - c.cxd) / c.fxd, aR = ((double)c.W + 0.5 - c.cxd) / c.fxd;
    const double aT = (-1.5 - c.cyd) / c.fyd, aB = ((double)c.H + 0.5 - c.cyd) / c.fyd;
    Frustum f;
    double n;
    n = sqrt(1.0 + aL * aL); f.lx = (float)(1.0 / n);  f.lz = (float)(-aL / n);
    n = sqrt(1.0 + aR * aR); f.rx = (float)(-1.0 / n); f.rz = (float)(aR / n);
    n = sqrt(1.0 + aT * aT); f.ty = (float)(1.0 / n);  f.tz = (float)(-aT / n);
    n = sqrt(1.0 + aB * aB); f.by = (float)(-1.0 / n); f.bz = (float)(aB / n);
    return f;
}

// ------------------------------------------------------------------------------------------- ordering around a slot's cache block
// every batch numbered b or lower has left the device: the host has waited since (tc_done_before), or the batch that is being
// issued waits for the scratch of batch (its number - TSDF_SCRATCHES) and every update before that one is ahead of it
static bool batch_known_complete(const tl3d_ctx *ctx, unsigned b) {
    return (int)(b - ctx->tc_done_before) < 0 || ctx->tsdf_batch_no - b >= (unsigned)TSDF_SCRATCHES;
}

// Who waits for whom around a product X kept in a slot's cache block (Cached: the tiles, Slot::tc, and the classification made from
// them, Slot::cc).  b = the number of the batch whose chain is being issued, h = b % TSDF_SCRATCHES, ps = its prep stream:
//   producer                                   event                        consumer
//   upload / ray cast into the slot (main;     Slot::ev_upload              everything of batch b on ps (flush_updates), the build of the
//     behind every earlier update, so behind                                  tiles with it.  slot_rewritten clears tc.valid and tc.used
//     every earlier user of the tiles)                                        and leaves cc alone: the rebuild that follows drops cc.valid
//   update of batch b - TSDF_SCRATCHES (main;  ev_upd[h], the scratch-reuse  everything of batch b on ps: covers every writer and user
//     it waited for that batch's chain)          wait of flush_updates         numbered b - TSDF_SCRATCHES or lower (batch_known_complete)
//   chain of batch w = X.write_batch,          ev_prep[w % TSDF_SCRATCHES]  a chain on ps that READS X (tiles: a hit; classification: a
//     b - 3 <= w < b, on another prep stream     (before_read)                replay); none if the host has waited since (tc_done_before)
//   update of batch u = X.use_batch,           ev_upd[u % TSDF_SCRATCHES]   a chain on ps that OVERWRITES X (tiles: a rebuild without an
//     b - 3 <= u < b, the last batch whose       (before_overwrite)           upload -- key change, cache off; classification: a new key,
//     chain read or wrote X                                                   masks added to a level-1 entry, or the masks of a level-2
//                                                                             entry refined: level 3).  u's update waited for
//                                                                             u's chain, and the updates before it for the chains of
//                                                                             earlier users; none if X.used is clear or the host has waited
//   chain of batch b (ps)                      ev_prep[h]                   update of batch b (main; flush_updates)
//   tl3d_count_bricks: chains on the main stream (behind every update, each of which waited for its chain: no wait), then a wait
//     for the stream: every later batch counts them complete (tc_done_before)
// The two look-ups of a chain share one ChainOrder, so an event both need is waited for once.  The update never touches the
// classification; a rebuild of the tiles drops it, and the next look-up writes it anew.  A slot twice in one chain: with one scale,
// one tile build, shared, and both uses replay a complete entry nothing in the chain writes (else the second is classified without
// the cache); with two scales the chain is cut in front of the second (chain_needs_cut).
struct ChainOrder {
    ChainOrder(tl3d_ctx *ctx, hipStream_t ps, unsigned batch) : ctx_(ctx), ps_(ps), batch_(batch), side_(ps != ctx->stream) {}
    int before_read(const Cached &x) {
        if (!side_ || batch_known_complete(ctx_, x.write_batch) || ctx_->prep_stream[x.write_batch % (unsigned)ctx_->n_prep_streams] == ps_) return TL3D_OK;
        const unsigned h = x.write_batch % (unsigned)TSDF_SCRATCHES;
        if (!((waited_prep_ >> h) & 1u)) TL3D_HIP(hipStreamWaitEvent(ps_, ctx_->ev_prep[h], 0));
        waited_prep_ |= 1u << h;
        return TL3D_OK;
    }
    int before_overwrite(const Cached &x) {
        if (!side_ || !x.used || batch_known_complete(ctx_, x.use_batch)) return TL3D_OK;
        const unsigned h = x.use_batch % (unsigned)TSDF_SCRATCHES;
        if (ctx_->upd_recorded[h] && !((waited_upd_ >> h) & 1u)) TL3D_HIP(hipStreamWaitEvent(ps_, ctx_->ev_upd[h], 0));
        waited_upd_ |= 1u << h;
        return TL3D_OK;
    }
    void wrote(Cached &x) const { x.valid = true; x.write_batch = batch_; }
    void used(Cached &x) const { x.used = true; x.use_batch = batch_; }
    tl3d_ctx *ctx_;
    hipStream_t ps_;
    unsigned batch_;
    bool side_;                                          // on the main stream nothing is waited for
    unsigned waited_prep_ = 0, waited_upd_ = 0;          // bit h: ps already waits for ev_prep[h] / ev_upd[h]
};

// ------------------------------------------------------------------------------------------- TSDF tile cache
// The tile buffers of the frames of chain c, which is about to be issued (ord: its stream and batch number), and which of the
// frames must build theirs (c.stale, appended).  A slot's tiles serve when the cache is on, they are built and their key (scale
// bits, depth limits) is the chain's; frames of one slot share one build (the caller has cut the chain where a slot would need
// two keys).  A build drops the slot's classification, which was made from the tiles it replaces.
static int tile_cache_lookup(tl3d_ctx *ctx, ChainOrder &ord, PrepChain &c) {
    size_t vt_off = 0, vp_off = 0;
    (void)tsdf_tile_cache_bytes(ctx->cam, &vt_off, &vp_off);
    for (int i = 0; i < c.n; ++i) {
        Slot &s = ctx->slots[c.slot[i]];
        if (!s.tiles) {
            char *p = (char *)pool_take(ctx->pool_tiles);
            if (!p) return set_err(TL3D_E_NOMEM, "tile cache alloc failed");
            s.tiles = (float4 *)p;
            s.vtile = (float2 *)(p + vt_off);
            s.vpix = (unsigned *)(p + vp_off);            // first word of the float4 behind the pyramid's last level
            s.cls = ctx->cc_bytes ? (unsigned *)(p + ctx->tc_bytes) : nullptr;
            s.tc = s.cc = Cached();
        }
        c.tiles[i] = s.tiles;
        bool shared = false;
        for (int j = 0; j < i && !shared; ++j) shared = c.slot[j] == c.slot[i];
        if (shared) { ctx->tc_hits++; continue; }
        uint32_t bits;
        memcpy(&bits, &c.scale[i], sizeof(bits));
        const bool hit = ctx->tile_cache && s.tc.valid && s.tc_scale_bits == bits && s.tc_mind == c.mind && s.tc_maxd == c.maxd;
        // (a rebuild behind an upload is ordered already: the upload sits behind every update, and ps waits for it)
        const int rc = hit ? ord.before_read(s.tc) : ord.before_overwrite(s.tc);
        if (rc) return rc;
        if (hit) {
            ctx->tc_hits++;
        } else {
            c.stale[c.n_stale++] = (unsigned char)i;
            s.cc.valid = false;
            s.tc_scale_bits = bits; s.tc_mind = c.mind; s.tc_maxd = c.maxd;
            ord.wrote(s.tc);
            ctx->tc_builds++;
        }
        ord.used(s.tc);
    }
    return TL3D_OK;
}
// a chain that was not issued (or not completely): its builds did not happen
static void tile_cache_forget(tl3d_ctx *ctx, const PrepChain &c) {
    for (int k = 0; k < c.n_stale; ++k) ctx->slots[c.slot[c.stale[k]]].tc.valid = false;
}

// ------------------------------------------------------------------------------------------- TSDF classification cache
static ClassKey class_key(const PoseF &p, float scale, float mind, float maxd, const Grid &g) {
    ClassKey k;
    const float f[20] = {p.r[0], p.r[1], p.r[2], p.r[3], p.r[4], p.r[5], p.r[6], p.r[7], p.r[8], p.t[0], p.t[1], p.t[2], scale, mind, maxd,
                         g.ox, g.oy, g.oz, g.vs, g.trunc};
    memcpy(k.w, f, sizeof(f));
    const int gi[6] = {g.nbx, g.nby, g.nbz, g.vox, g.voy, g.voz};
    memcpy(k.w + 20, gi, sizeof(gi));
    return k;
}

// How the classification kernels of the chain that tile_cache_lookup has just prepared treat each of its frames (c.plan), and
// which slots' entries the chain writes (c.class_writes: bit i = frame i's; class_finish_kernel must run, class_cache_forget
// undoes it).  A slot's entry serves when the cache is on, the entry is valid -- no tile rebuild since it was made, this
// chain's included -- and its key is the frame's, bit for bit: the frame is REPLAYED (if it fit: the device knows).  Otherwise
// the frame is classified and SAVED under its key.  A classify-only chain asks for level 1; a fusion that finds level 1 replays
// it, classifies the sub-bricks and leaves level 2, which counts as a write.  A fusion that finds level 2 replays it and -- if
// refinement is on (TL3D_CLASS_REFINE), the chain holds the slot once and has not reached CLASS_REFINES_PER_CHAIN -- refines the
// masks and leaves level 3 (plan.refine; a write of the same kind: before_overwrite, class_writes, wrote).  Lazy on purpose: a
// frame that is fused once, and count-then-fuse, pay nothing.  Level 3 serves every chain as level 2 does.  One slot twice in a
// chain: the second use is a replay if the first is one that writes nothing and the keys are equal, else it is classified
// without the cache; such a chain refines nothing of that slot.
// A chain refines at most this many of its frames' entries; the others stay at level 2 until the next chain that replays them.  The
// refinement of 32 frames is as much work as their update, and what does not fit beside the update on the prep streams delays it:
// plain bench.py, whose first timed steps refine, ran 1.1 % under the parent with 16 per chain, 1.2-1.3 % over it with 8 or 4.
constexpr int CLASS_REFINES_PER_CHAIN = 8;
static int class_cache_lookup(tl3d_ctx *ctx, ChainOrder &ord, PrepChain &c, const Grid &g, bool classify_only) {
    ClassPlan &plan = c.plan;
    memset(&plan, 0, sizeof(plan));
    plan.cap = ctx->cc_entries;
    plan.stats = ctx->d_cc_stats;
    if (!ctx->class_cache || !ctx->tile_cache) return TL3D_OK;      // every frame: CC_CLASSIFY
    int n_refines = 0;
    for (int i = 0; i < c.n; ++i) {
        Slot &s = ctx->slots[c.slot[i]];
        const ClassKey key = class_key(c.pose[i], c.scale[i], c.mind, c.maxd, g);
        int first = -1;
        for (int j = 0; j < i && first < 0; ++j)
            if (c.slot[j] == c.slot[i]) first = j;
        if (first >= 0) {
            if (class_mode(plan, first) == CC_REPLAY && !((c.class_writes >> first) & 1u) && memcmp(&key, &s.cc_key, sizeof(key)) == 0) {
                class_set_mode(plan, i, CC_REPLAY);
                plan.cache[i] = s.cls;
            }
            continue;
        }
        if (!s.cls) return set_err(TL3D_E_STATE, "slot %d has no classification buffer", c.slot[i]);      // (it comes with the tiles: tile_cache_lookup)
        plan.cache[i] = s.cls;
        const bool hit = s.cc.valid && memcmp(&key, &s.cc_key, sizeof(key)) == 0;
        // the first fusion chain that replays a level-2 entry refines its masks (class_refine_kernel) -- if it holds the slot once:
        // a second use in the chain would read the masks while they change
        bool refines = hit && !classify_only && s.cc_level == 2 && ctx->class_refine && n_refines < CLASS_REFINES_PER_CHAIN;
        for (int j = i + 1; j < c.n && refines; ++j) refines = c.slot[j] != c.slot[i];
        const bool reads = hit && (classify_only || s.cc_level >= 2) && !refines;    // else a write: a save under a new key, level 1 -> 2, or 2 -> 3
        const int rc = reads ? ord.before_read(s.cc) : ord.before_overwrite(s.cc);
        if (rc) return rc;
        if (reads) {
            class_set_mode(plan, i, CC_REPLAY);
        } else {
            class_set_mode(plan, i, hit ? CC_REPLAY : CC_SAVE);
            c.class_writes |= 1u << i;
            if (refines) { plan.refine |= 1u << i; ++n_refines; }
            s.cc_key = key;
            s.cc_level = classify_only ? 1 : refines ? 3 : 2;
            ord.wrote(s.cc);
        }
        ord.used(s.cc);
    }
    return TL3D_OK;
}
// a chain that was not issued (or not completely): what it was to write is not there
static void class_cache_forget(tl3d_ctx *ctx, const PrepChain &c) {
    for (int i = 0; i < c.n; ++i)
        if ((c.class_writes >> i) & 1u) ctx->slots[c.slot[i]].cc.valid = false;
}

// ------------------------------------------------------------------------------------------- a prep chain
// one set of tiles per slot in a chain: does frame (slot, scale) need a new chain, given the n frames c has collected?
static bool chain_needs_cut(const PrepChain &c, int n, int slot, float scale) {
    for (int i = 0; i < n; ++i)
        if (c.slot[i] == slot && memcmp(&c.scale[i], &scale, sizeof(float)) != 0) return true;
    return false;
}
static void chain_set(PrepChain &c, int i, int slot, const PoseF &pose, float scale, const void *depth) {
    c.slot[i] = slot; c.pose[i] = pose; c.scale[i] = scale; c.depth[i] = depth;
}

// The prep chain of the frames collected in c on stream ps, as batch number `batch`, against grid g: both look-ups, which order ps
// behind what the chain must not overtake, then the launches.  On failure the slots forget what the chain was to leave in them.
static int issue_prep_chain(tl3d_ctx *ctx, hipStream_t ps, unsigned batch, PrepChain &c, const Grid &g, int max_frames, void *scratch, unsigned *free_cnt,
                            bool classify_only) {
    ChainOrder ord(ctx, ps, batch);
    c.n_stale = 0; c.class_writes = 0u;
    int rc = tile_cache_lookup(ctx, ord, c);
    if (!rc) rc = class_cache_lookup(ctx, ord, c, g, classify_only);
    if (!rc) rc = launch_tsdf_prepare(ps, ctx->cam, g, make_frustum(ctx->cam), c, max_frames, scratch, free_cnt, classify_only);
    if (!rc && c.plan.modes == 0ull) ctx->cc_classified_host += (unsigned long long)c.n;     // (such a chain's kernels do not count)
    if (rc) {
        tile_cache_forget(ctx, c);
        class_cache_forget(ctx, c);
    }
    return rc;
}

static int ktimer_begin(tl3d_ctx *ctx) {
    if (!ctx->time_kernels) return -1;
    if (!ctx->ktimers) {
        ctx->n_ktimers = 1024;
        ctx->ktimers = new (std::nothrow) tl3d_ctx::KTimer[ctx->n_ktimers];
        if (!ctx->ktimers) return -1;
        for (int i = 0; i < ctx->n_ktimers; ++i) {
            (void)hipEventCreate(&ctx->ktimers[i].a);
            (void)hipEventCreate(&ctx->ktimers[i].b);
        }
        ctx->ktimers_used = 0;
    }
    if (ctx->ktimers_used == ctx->n_ktimers) {          // drain
        (void)hipStreamSynchronize(ctx->stream);
        for (int i = 0; i < ctx->ktimers_used; ++i) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ctx->ktimers[i].a, ctx->ktimers[i].b) == hipSuccess) {
                ctx->stats.tsdf_kernel_ms += ms;
                ctx->stats.tsdf_kernel_timed += (uint64_t)ctx->ktimers[i].launches;
            }
        }
        ctx->ktimers_used = 0;
    }
    const int id = ctx->ktimers_used++;
    (void)hipEventRecord(ctx->ktimers[id].a, ctx->stream);
    return id;
}

// the pending voxel-centroid accumulations: one launch for all of them (they share a stride)
static int flush_centroid(tl3d_ctx *ctx) {
    if (ctx->n_cen_pend == 0) return TL3D_OK;
    const int n = ctx->n_cen_pend;
    ctx->n_cen_pend = 0;                                // whatever happens below, the batch is consumed
    TL3D_HIP(hipSetDevice(ctx->device));
    if (!ctx->d_cen_frames && hipMalloc(&ctx->d_cen_frames, sizeof(CenFrame) * TL3D_CEN_MAXBATCH) != hipSuccess)
        return set_err(TL3D_E_NOMEM, "centroid descriptor alloc failed");
    ctx->grid_epoch++;
    const int rc = launch_centroid_batch(ctx->stream, ctx->cam, ctx->grid, n, ctx->cen_pend, ctx->d_cen_frames, ctx->bp_factors, ctx->bp_factors + ctx->cam.W,
                                         ctx->centroid, ctx->d_cen_counters);
    if (rc) return rc;
    ctx->stats.centroid_launches++;
    return TL3D_OK;
}

// Issues the pending batch: its prep chain on a side stream (it needs the frames' uploads, the batch scratch whose previous
// user -- TSDF_SCRATCHES batches ago -- has been updated, and the last clear / fold of the free-space counters; what it needs
// around the slots' caches is ChainOrder's), then ONE update launch on the main stream behind it.  Results never depend on where the
// batch boundaries fall (integer sums).
int tl3d::flush_updates(tl3d_ctx *ctx) {
    const int crc = flush_centroid(ctx);
    if (crc) return crc;
    if (ctx->n_pend == 0) return TL3D_OK;
    ctx->grid_epoch++;
    TL3D_HIP(hipSetDevice(ctx->device));
    PrepChain &c = ctx->pend;
    c.n = ctx->n_pend;
    ctx->n_pend = 0;                                    // whatever happens below, the batch is consumed
    c.mind = (float)ctx->cfg.min_depth; c.maxd = (float)ctx->cfg.max_depth;
    const int half = (int)(ctx->tsdf_batch_no % (unsigned)TSDF_SCRATCHES);
    hipStream_t ps = ctx->tsdf_single_stream ? ctx->stream : ctx->prep_stream[ctx->tsdf_batch_no % (unsigned)ctx->n_prep_streams];
    if (ps != ctx->stream) {
        for (int i = 0; i < c.n; ++i)
            if (ctx->slots[c.slot[i]].ev_upload) TL3D_HIP(hipStreamWaitEvent(ps, ctx->slots[c.slot[i]].ev_upload, 0));
        if (ctx->upd_recorded[half]) TL3D_HIP(hipStreamWaitEvent(ps, ctx->ev_upd[half], 0));
        if (ctx->ev_free_recorded) TL3D_HIP(hipStreamWaitEvent(ps, ctx->ev_free, 0));      // clears / folds of the free-space counters
    }
    int rc = issue_prep_chain(ctx, ps, ctx->tsdf_batch_no, c, ctx->grid, ctx->tsdf_batch, ctx->tsdf_scratch[half], ctx->free_cnt, false);
    if (rc) return rc;
    if (ps != ctx->stream) {
        TL3D_HIP(hipEventRecord(ctx->ev_prep[half], ps));
        TL3D_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_prep[half], 0));
    }
    // profiling mode: one event pair around the update kernel
    const int kt = ktimer_begin(ctx);
    rc = launch_tsdf_update(ctx->stream, ctx->cam, ctx->grid, c.n, ctx->tsdf_batch, c.depth_u16, c.mind, c.maxd, ctx->tsdf, ctx->tsdf_scratch[half],
                            ctx->d_counters, ctx->count_records, ctx->tsdf_max_blocks);
    if (rc == TL3D_OK) ctx->stats.tsdf_launches++;
    if (kt >= 0) {
        ctx->ktimers[kt].launches = rc == TL3D_OK ? 1 : 0;
        (void)hipEventRecord(ctx->ktimers[kt].b, ctx->stream);
    }
    ctx->tsdf_batch_no++;
    TL3D_HIP(hipEventRecord(ctx->ev_upd[half], ctx->stream));
    ctx->upd_recorded[half] = true;
    return rc;
}

extern "C" {

// ------------------------------------------------------------------------------------------- occupancy of a planned grid
// Which bricks of a grid (geometry only: no records, no pools) a fusion of these frames WOULD give records to: the TSDF
// classification of every frame (tiles, pyramid, brick classes: the update's own prep chain, sub-brick masks and update left out)
// and the bricks the frames' samples fall into, against scratch brick tables whose cursors count the distinct bricks.  What a
// sparse grid's pools must hold (tl3d_config.pool_bricks_*): the reference's hash-map merge sizes itself (D2R:404-410); a pool is
// allocated up front, and this is how to know how large -- a few microseconds per frame instead of a guess.
int tl3d_count_bricks(tl3d_ctx *ctx, const tl3d_config *cfg, int n_frames, const int32_t *slots, const double *R, const double *t,
                      const double *scales, int centroid_subsample, double min_depth, double max_depth, int64_t *bricks_tsdf,
                      int64_t *bricks_centroid) {
    REQUIRE(ctx && cfg && slots && R && t && bricks_tsdf && bricks_centroid, TL3D_E_INVALID, "null argument");
    REQUIRE(n_frames >= 1, TL3D_E_INVALID, "n_frames must be positive");
    int rc = validate_grid(cfg);
    if (rc) return rc;
    for (int i = 0; i < n_frames; ++i) {
        rc = check_slot(ctx, slots[i], true);
        if (rc) return rc;
    }
    FLUSH_UPDATES(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    Grid g;
    memset(&g, 0, sizeof(g));
    grid_geometry(g, cfg);
    const size_t nbr = ((size_t)g.nx * g.ny * g.nz) >> 9;
    Staging st(ctx);                                    // the temporaries below go when the call returns, behind the stream
    unsigned *tabs, *free_cnt = nullptr;
    void *scratch = nullptr;
    rc = st.scratch((2 * nbr + 64) * sizeof(unsigned), &tabs);
    if (rc) return rc;
    TL3D_HIP(hipMemsetAsync(tabs, 0xff, 2 * nbr * sizeof(unsigned), ctx->stream));
    TL3D_HIP(hipMemsetAsync(tabs + 2 * nbr, 0, 64 * sizeof(unsigned), ctx->stream));
    g.tsdf_tab = tabs; g.cen_tab = tabs + nbr; g.cursors = tabs + 2 * nbr;
    g.tsdf_cap = g.cen_cap = (unsigned)nbr;
    if (cfg->channels & TL3D_CH_TSDF) {
        const int batch = TL3D_TSDF_MAXBATCH;
        const size_t sb = tsdf_batch_scratch_bytes(ctx->cam, g, batch);
        rc = st.scratch(nbr * sizeof(unsigned), &free_cnt);
        if (!rc) rc = st.scratch(sb, &scratch);
        if (rc) return rc;
        size_t zoff = 0, zbytes = 0;
        tsdf_batch_scratch_zero_range(ctx->cam, g, batch, &zoff, &zbytes);
        TL3D_HIP(hipMemsetAsync(free_cnt, 0, nbr * sizeof(unsigned), ctx->stream));
        // The chains run on the main stream, behind every update issued so far: the tiles they find are complete, the ones they
        // build overwrite nothing a batch still reads, and the call ends with a wait for the stream -- numbered as the last issued
        // batch they count as complete from then on.
        PrepChain c;
        c.depth_u16 = false; c.mind = (float)min_depth; c.maxd = (float)max_depth;      // (always the f32 image)
        for (int i0 = 0; i0 < n_frames; i0 += c.n) {
            for (c.n = 0; c.n < batch && i0 + c.n < n_frames; ++c.n) {
                const int i = i0 + c.n;
                const float sc = (float)(scales ? scales[i] : 1.0);
                if (chain_needs_cut(c, c.n, slots[i], sc)) break;
                chain_set(c, c.n, slots[i], make_pose_f(R + (size_t)9 * i, t + (size_t)3 * i), sc, ctx->slots[slots[i]].depth);
            }
            rc = hipMemsetAsync((char *)scratch + zoff, 0, zbytes, ctx->stream) != hipSuccess ? set_err(TL3D_E_HIP, "memset failed") : TL3D_OK;    // (no update re-arms the frame masks)
            if (!rc) rc = issue_prep_chain(ctx, ctx->stream, ctx->tsdf_batch_no - 1u, c, g, batch, scratch, free_cnt, true);
            if (rc) {
                (void)hipStreamSynchronize(ctx->stream);
                ctx->tc_done_before = ctx->tsdf_batch_no;
                return rc;
            }
        }
    }
    if ((cfg->channels & TL3D_CH_CENTROID) && centroid_subsample >= 1) {
        for (int i = 0; i < n_frames; ++i) {
            BpArgs a;
            rc = make_bp_args(ctx, scales ? scales[i] : 1.0, 0, centroid_subsample, min_depth, max_depth, &a);
            if (rc) return rc;
            const PoseD p = make_pose_d(R + (size_t)9 * i, t + (size_t)3 * i, false);
            rc = launch_centroid_mark(ctx->stream, ctx->cam, g, a, p, ctx->slots[slots[i]].depth, ctx->bp_factors, ctx->bp_factors + ctx->cam.W);
            if (rc) return rc;
        }
    }
    unsigned cur[4] = {0, 0, 0, 0};
    TL3D_HIP(hipMemcpyAsync(cur, g.cursors, sizeof(cur), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    ctx->tc_done_before = ctx->tsdf_batch_no;
    *bricks_tsdf = (int64_t)(cur[0] < nbr ? cur[0] : nbr);
    *bricks_centroid = (int64_t)(cur[2] < nbr ? cur[2] : nbr);
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- centroid accumulation
int tl3d_accumulate_centroid(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale, uint32_t flags,
                             int subsample, double min_depth, double max_depth) {
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    REQUIRE(ctx->centroid != nullptr, TL3D_E_STATE, "centroid channel not enabled");
    REQUIRE((flags & TL3D_F_NO_POSE) || (R && t), TL3D_E_INVALID, "pose required unless TL3D_F_NO_POSE");
    BpArgs a;
    rc = make_bp_args(ctx, scale, flags, subsample, min_depth, max_depth, &a);
    if (rc) return rc;
    const Slot &s = ctx->slots[slot];
    // The frame joins the pending batch (one stride per batch); the batch goes out when it is full, or when any call needs the grid,
    // a slot, a sync or a time stamp (flush_updates).  Integer sums: the grid does not depend on where the batches are cut.
    if (ctx->n_cen_pend > 0 && ctx->cen_pend[0].a.sub != a.sub) {
        rc = flush_centroid(ctx);
        if (rc) return rc;
    }
    CenFrame &f = ctx->cen_pend[ctx->n_cen_pend++];
    f.p = make_pose_d(R, t, (flags & TL3D_F_NO_POSE) != 0);
    f.a = a;
    f.depth = s.depth;
    f.bgr = s.has_color ? s.bgr : nullptr;
    if (ctx->n_cen_pend >= TL3D_CEN_MAXBATCH) return flush_centroid(ctx);
    return TL3D_OK;
}

int tl3d_accumulate_points(tl3d_ctx *ctx, const float *xyz, const uint8_t *rgb, int64_t n) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(ctx->centroid != nullptr, TL3D_E_STATE, "centroid channel not enabled");
    REQUIRE(n >= 0 && (n == 0 || (xyz && rgb)), TL3D_E_INVALID, "bad point list");
    if (n == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *dxyz;
    const uint8_t *drgb;
    int rc = st.in(xyz, (size_t)n * 12, &dxyz);
    if (!rc) rc = st.in(rgb, (size_t)n * 3, &drgb);
    if (rc) return rc;
    ctx->grid_epoch++;
    rc = st.finish(launch_centroid_points(ctx->stream, ctx->grid, dxyz, drgb, n, ctx->centroid, ctx->d_cen_counters));
    if (rc) return rc;
    ctx->stats.centroid_launches++;
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- TSDF
int tl3d_integrate(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale) {
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    REQUIRE(ctx->tsdf != nullptr, TL3D_E_STATE, "TSDF channel not enabled");
    REQUIRE(R && t, TL3D_E_INVALID, "null pose");
    TL3D_HIP(hipSetDevice(ctx->device));
    const PoseF p = make_pose_f(R, t);
    // int32 headroom: one more observation must keep every |sum_q| <= weight * 32767 below 2^31
    if (ctx->tsdf_w_unknown || ctx->tsdf_w_upper + 1 > TL3D_TSDF_MAX_WEIGHT) {
        FLUSH_AND_FOLD(ctx);
        long long w = 0;
        rc = measure_max_weight(ctx, ctx->tsdf, &w);
        if (rc) return rc;
        ctx->tsdf_w_upper = w;
        ctx->tsdf_w_unknown = false;
        REQUIRE(w + 1 <= TL3D_TSDF_MAX_WEIGHT, TL3D_E_STATE,
                "a voxel already holds %lld observations: one more could overflow its int32 TSDF sum (limit %d); extract or reset the grid",
                w, TL3D_TSDF_MAX_WEIGHT);
    }
    ctx->tsdf_w_upper++;
    ctx->free_dirty = true;
    const Slot &sl = ctx->slots[slot];
    const bool u16 = sl.has_u16 && ctx->tsdf_use_u16;
    // The frame joins the pending batch (one depth kind per batch, and one set of tiles per slot); the batch goes out when it is
    // full, or when any call needs the grid, a slot, a sync or a time stamp (flush_updates): the slot's images stay until then.
    PrepChain &c = ctx->pend;
    if (ctx->n_pend > 0 && c.depth_u16 != u16) FLUSH_UPDATES(ctx);
    if (chain_needs_cut(c, ctx->n_pend, slot, (float)scale)) FLUSH_UPDATES(ctx);
    c.depth_u16 = u16;
    chain_set(c, ctx->n_pend++, slot, p, (float)scale, u16 ? (const void *)sl.depth_u16 : (const void *)sl.depth);
    if (ctx->n_pend >= (ctx->tsdf_pairing ? ctx->tsdf_batch : 1)) return flush_updates(ctx);
    return TL3D_OK;
}

int tl3d_tile_cache_info(tl3d_ctx *ctx, uint64_t *builds, uint64_t *hits, uint64_t *bytes) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    FLUSH_UPDATES(ctx);                                 // (look-ups happen when a batch is issued)
    if (builds) *builds = ctx->tc_builds;
    if (hits) *hits = ctx->tc_hits;
    if (bytes) *bytes = (uint64_t)(ctx->cfg.n_slots - ctx->pool_tiles.remaining) * ctx->tc_bytes;
    return TL3D_OK;
}

int tl3d_class_cache_info(tl3d_ctx *ctx, uint64_t *classified, uint64_t *replayed, uint64_t *overflowed, uint64_t *bytes) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    FLUSH_UPDATES(ctx);                                 // (look-ups happen when a batch is issued)
    TL3D_HIP(hipSetDevice(ctx->device));
    // which path a frame took is the device's decision (only it knows whether the frame fit): its counters, behind every update
    // issued so far and so behind every chain
    unsigned long long h[4] = {0, 0, 0, 0};
    TL3D_HIP(hipMemcpyAsync(h, ctx->d_cc_stats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    if (classified) *classified = h[0] + ctx->cc_classified_host;
    if (replayed) *replayed = h[1];
    if (overflowed) *overflowed = h[2];
    if (bytes) *bytes = (uint64_t)(ctx->cfg.n_slots - ctx->pool_tiles.remaining) * ctx->cc_bytes;
    return TL3D_OK;
}

int tl3d_class_refine_info(tl3d_ctx *ctx, uint64_t *seen, uint64_t *dropped, uint64_t *freed, uint64_t *decided, uint64_t *overflowed) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    FLUSH_UPDATES(ctx);                                 // (look-ups happen when a batch is issued)
    TL3D_HIP(hipSetDevice(ctx->device));
    // the refinement's own counters (class_refine_kernel), behind every update issued so far and so behind every chain
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    TL3D_HIP(hipMemcpyAsync(h, ctx->d_cc_stats + 4, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    if (seen) *seen = h[0];
    if (dropped) *dropped = h[1];
    if (freed) *freed = h[2];
    if (decided) *decided = h[3];
    if (overflowed) *overflowed = h[4];
    return TL3D_OK;
}

int tl3d_fuse_frames(tl3d_ctx *ctx, int n, const int32_t *slots, const double *R, const double *t, const double *scales,
                     uint32_t flags, int centroid_subsample, double min_depth, double max_depth) {
    REQUIRE(ctx && slots && R && t, TL3D_E_INVALID, "null argument");
    REQUIRE(n >= 0, TL3D_E_INVALID, "n must not be negative");
    for (int i = 0; i < n; ++i) {
        const double sc = scales ? scales[i] : 1.0;
        if (ctx->tsdf) {
            const int rc = tl3d_integrate(ctx, slots[i], R + (size_t)9 * i, t + (size_t)3 * i, sc);
            if (rc) return rc;
        }
        if (ctx->centroid && centroid_subsample >= 1) {
            const int rc = tl3d_accumulate_centroid(ctx, slots[i], R + (size_t)9 * i, t + (size_t)3 * i, sc, flags, centroid_subsample, min_depth, max_depth);
            if (rc) return rc;
        }
    }
    return TL3D_OK;
}

}  // extern "C"
