// Graph plan: everything about one (edge list, batch ids, point count) that does not depend on the tensors' values --
// scene partition, CSR over sources, attention tile tables, one device arena carved into every workspace buffer.  What of that is
// host arithmetic (the analysis, the list of the arena's buffers and their layout) is plan_graph.h; here are the HIP objects.
//
// No device-wide synchronisation anywhere on this path: the index tables are packed into ONE pinned host
// buffer and uploaded with ONE hipMemcpyAsync on the handle's copy stream; the first forward of the plan makes its
// stream wait for that upload's event.  A destroyed plan hands its arena to the pool together with the event of the
// last forward that touched it; whoever takes the arena next orders its upload behind that event, and arenas that
// fall out of the pool are only freed once the event has completed.
#include <algorithm>
#include <cstring>
#include <memory>

#include "engine.h"

using namespace vlsat;

namespace vlsat {

hipEvent_t take_event(vlsat_ctx* h) {
    if (!h->spare_ev.empty()) {
        hipEvent_t e = h->spare_ev.back();
        h->spare_ev.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return e;
}
void give_event(vlsat_ctx* h, hipEvent_t e) {
    if (e) h->spare_ev.push_back(e);
}

// arenas that fell out of the pool: free those whose last forward has completed (hipFree may block on the device,
// so never call it on memory that is still in use)
static void sweep_trash(vlsat_ctx* h, bool force) {
    for (size_t i = 0; i < h->arena_trash.size();) {
        Arena& a = h->arena_trash[i];
        if (force || !a.last || hipEventQuery(a.last) == hipSuccess) {
            hipFree(a.p);
            give_event(h, a.last);
            h->arena_trash.erase(h->arena_trash.begin() + i);
        } else {
            ++i;
        }
    }
}

void release_plan_resources(vlsat_ctx* h) {
    sweep_trash(h, true);
    for (auto& a : h->arena_pool) { hipFree(a.p); if (a.last) hipEventDestroy(a.last); }
    h->arena_pool.clear();
    for (auto& s : h->staging) { hipHostFree(s.p); if (s.done) hipEventDestroy(s.done); }
    h->staging.clear();
    for (hipEvent_t e : h->spare_ev) hipEventDestroy(e);
    h->spare_ev.clear();
}

// a pinned buffer of at least `bytes` whose previous upload has completed
static int take_staging(vlsat_ctx* h, size_t bytes, Staging** out) {
    for (auto& s : h->staging)
        if (s.bytes >= bytes && hipEventQuery(s.done) == hipSuccess) { *out = &s; return 0; }
    if (h->staging.size() >= 16) {              // all busy (16 uploads in flight): wait for the oldest that fits, else the first
        Staging* pick = &h->staging[0];
        for (auto& s : h->staging) if (s.bytes >= bytes) { pick = &s; break; }
        VLSAT_HIP_CHECK(hipEventSynchronize(pick->done));
        if (pick->bytes < bytes) {
            hipHostFree(pick->p);
            pick->p = nullptr;
            pick->bytes = std::max<size_t>(bytes * 2, 1 << 16);
            VLSAT_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&pick->p), pick->bytes, hipHostMallocDefault));
        }
        *out = pick;
        return 0;
    }
    Staging s;
    s.bytes = std::max<size_t>(bytes * 2, 1 << 16);
    VLSAT_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&s.p), s.bytes, hipHostMallocDefault));
    VLSAT_HIP_CHECK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    h->staging.push_back(s);
    *out = &h->staging.back();
    return 0;
}

static PlanCfg plan_cfg_of(const vlsat_ctx* h) {
    PlanCfg c;
    c.H = h->H; c.D = h->D; c.A = h->A;
    c.edge_scope = h->edge_scope; c.fa_split = h->fa_split; c.flash_bq_big_min = h->flash_bq_big_min; c.dual_stream = h->dual_stream;
    c.n_layers = h->d.n_layers; c.n_obj_class = h->d.n_obj_class; c.n_rel_class = h->d.n_rel_class; c.feature_transform = h->d.feature_transform;
    return c;
}
static_assert(sizeof(PlanTile) == sizeof(int4) && alignof(PlanTile) == alignof(int4), "the tile tables are uploaded as bytes");

}  // namespace vlsat

extern "C" {

int vlsat_plan_create(vlsat_handle h, const int64_t* bid, const int64_t* edges, int64_t N, int64_t E, int32_t P,
                      vlsat_plan* out) {
    if (!h || !out || !bid || (!edges && E > 0)) return fail(VLSAT_EINVAL, "vlsat_plan_create: null argument");
    if (!h->finalized) return fail(VLSAT_ESTATE, "weights not finalised");
    if (N <= 0 || E < 0 || P <= 0) return fail(VLSAT_EINVAL, "N, P must be positive and E non-negative");
    if (N > (1 << 28) || E > (1ll << 30)) return fail(VLSAT_EINVAL, "graph too large for 32-bit indices");
    // ---- the graph, then the workspace it needs: host arithmetic alone (plan_graph.h) ----
    const PlanCfg cfg = plan_cfg_of(h);
    PlanGraph g = plan_graph_analyse(bid, edges, N, E, cfg);
    if (g.code) return fail(g.code, g.error);
    const WsLayout L = ws_layout(ws_params(cfg, g, N, E, P));
    std::unique_ptr<vlsat_plan_s> p(new vlsat_plan_s());
    p->h = h; p->N = N; p->E = E; p->P = P;
    p->S = g.S; p->max_n = g.max_n; p->max_e = g.max_e; p->is_fc = g.is_fc;
    p->n_tiles = (int)g.tiles.size(); p->n_tiles_big = (int)g.tiles_big.size(); p->fa_parts = g.fa_parts; p->flash_flops = g.flash_flops;
    p->ws = L.w; p->dual = L.w.dual; p->kvx_slots = (int)L.w.kvx_slots();
    p->stn_ws_floats = L.bytes[WS_stn_ws] / sizeof(float);
    p->ws_bytes = L.total;
    // ---- an arena: a pooled one that fits, else a fresh one of the next size class ----
    sweep_trash(h, false);
    hipEvent_t prev_use = nullptr;
    const int best = arena_pool_pick(h->arena_pool, L.total);
    if (best >= 0) {
        p->arena = h->arena_pool[best].p;
        p->arena_bytes = h->arena_pool[best].bytes;
        prev_use = h->arena_pool[best].last;
        h->arena_pool.erase(h->arena_pool.begin() + best);
    } else {
        p->arena_bytes = arena_size_class(L.total);
        VLSAT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p->arena), p->arena_bytes));
    }
    ws_carve(p.get(), p->arena, L);
    p->prob = nullptr;
    // ---- pack the index tables + one asynchronous upload ----
    auto give_up = [&](int code, const std::string& msg) {
        h->arena_pool.push_back({p->arena, p->arena_bytes, prev_use});
        p->arena = nullptr;
        return fail(code, msg);
    };
    if (!h->copy && hipStreamCreateWithFlags(&h->copy, hipStreamNonBlocking) != hipSuccess)
        return give_up(VLSAT_EHIP, "plan: cannot create the copy stream");
    Staging* st = nullptr;
    if (take_staging(h, L.index_bytes, &st)) return give_up(VLSAT_EHIP, std::string("plan staging: ") + vlsat_last_error());
    pack_index_tables(g, L, st->p);
    p->uploaded = take_event(h);
    p->last_use = take_event(h);
    hipError_t er = (p->uploaded && p->last_use) ? hipSuccess : hipErrorOutOfMemory;
    if (er == hipSuccess && prev_use) er = hipStreamWaitEvent(h->copy, prev_use, 0);     // the arena's previous owner is done
    if (er == hipSuccess) er = hipMemcpyAsync(p->arena, st->p, L.index_bytes, hipMemcpyHostToDevice, h->copy);
    if (er == hipSuccess) er = hipEventRecord(st->done, h->copy);
    if (er == hipSuccess) er = hipEventRecord(p->uploaded, h->copy);
    if (er != hipSuccess) {
        give_event(h, p->uploaded); give_event(h, p->last_use);
        return give_up(VLSAT_EHIP, std::string("plan upload: ") + hipGetErrorString(er));
    }
    give_event(h, prev_use);       // (stream-ordered: the wait above has been enqueued; the handle may re-record it later)
    p->upload_pending = true;
    p->node_ptr = std::move(g.node_ptr); p->edge_ptr = std::move(g.edge_ptr);
    *out = p.release();
    return 0;
}

void vlsat_plan_destroy(vlsat_plan p) {
    if (!p) return;
    vlsat_ctx* h = p->h;
    if (p->arena) {
        // The forward that used this workspace may still be in flight: the arena keeps the event of that forward (or
        // of the upload, if the plan never ran) and whoever takes it next waits for it ON THE DEVICE.  No host wait.
        Arena a{p->arena, p->arena_bytes, p->used ? p->last_use : p->uploaded};
        give_event(h, p->used ? p->uploaded : p->last_use);
        // the pool is bounded by bytes (8 GiB of 288) and count; beyond that the largest pooled arena goes
        h->arena_pool.push_back(a);
        size_t pooled = 0;
        for (auto& x : h->arena_pool) pooled += x.bytes;
        while (h->arena_pool.size() > 1 && (pooled > (size_t(8) << 30) || h->arena_pool.size() > 64)) {
            size_t big = 0;
            for (size_t i = 1; i < h->arena_pool.size(); ++i) if (h->arena_pool[i].bytes > h->arena_pool[big].bytes) big = i;
            pooled -= h->arena_pool[big].bytes;
            h->arena_trash.push_back(h->arena_pool[big]);
            h->arena_pool.erase(h->arena_pool.begin() + big);
        }
        sweep_trash(h, false);
    }
    delete p;
}

int vlsat_plan_info(vlsat_plan p, int32_t* n_scenes, size_t* ws, int32_t* is_fc) {
    if (!p) return fail(VLSAT_EINVAL, "null plan");
    if (n_scenes) *n_scenes = p->S;
    if (ws) *ws = p->ws_bytes;
    if (is_fc) *is_fc = p->is_fc;
    return 0;
}

// Does a DEVICE copy of the graph equal what this plan was built from?  *mismatches (device int32, zeroed by the caller) gets the
// number of edge columns of edges_dev [2,E] (int64) that differ from the plan's (from, to) tables plus the nodes at which
// batch_ids_dev (int64 [N], may be NULL) starts a run where the plan has no scene boundary or vice versa.  Asynchronous on
// `stream`.  For callers that name a graph by a key instead of handing the edge list over the host (VLSATModel's `fc_sizes`
// hint with device tensors): one call per new key makes the key's claim checked instead of trusted -- a wrongly ordered edge
// list would otherwise attribute every rel_cls row to the wrong edge (reference edge order: dataset_3dssg.py:264-266).
int vlsat_plan_check_graph(vlsat_plan p, const int64_t* edges_dev, const int64_t* batch_ids_dev, int32_t* mismatches, void* stream) {
    if (!p || !mismatches || (p->E > 0 && !edges_dev)) return fail(VLSAT_EINVAL, "vlsat_plan_check_graph: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p->upload_pending) {               // the plan's tables travel on the handle's copy stream
        VLSAT_HIP_CHECK(hipStreamWaitEvent(s, p->uploaded, 0));
        if (hipEventQuery(p->uploaded) == hipSuccess) p->upload_pending = false;
    }
    RUN(launch_check_graph(edges_dev, p->E, p->d_src, p->d_dst, batch_ids_dev, p->N, p->d_scene_ptr, p->S, mismatches, s));
    p->used = true;                        // (the arena's next owner must order behind this read)
    VLSAT_HIP_CHECK(hipEventRecord(p->last_use, s));
    return 0;
}

// debug: device pointer / shape of a named workspace buffer of a plan
int vlsat_debug_buffer(vlsat_plan p, const char* name, void** ptr, int64_t* rows, int32_t* cols, int32_t* ld) {
    if (!p || !name) return fail(VLSAT_EINVAL, "null argument");
    struct B { const char* n; void* p; int64_t r; int c, ld; };
    const WsParams& w = p->ws;
    const int LDX = (int)w.LDX, A = (int)w.A;
    // the buffers whose row of the list states visible columns (a flat one shows as one row without columns), and two views of the aggregated message
    auto n_rows = [&](WsRows r) { return r == WS_NODES ? p->N : r == WS_EDGES ? p->E : 1; };
#define VLSAT_WS_DEBUG(m, T, r, per, when, cols) {#m, p->m, n_rows(r), cols, cols > 0 ? (int)(per) : 0},
    const B tab[] = {VLSAT_WS_BUFFERS(VLSAT_WS_DEBUG){"AGG3", p->X3 + 512, p->N, A, LDX}, {"AGG2", p->X2 + 512, p->N, A, LDX}};
#undef VLSAT_WS_DEBUG
    for (auto& b : tab)
        if (b.c >= 0 && !std::strcmp(b.n, name)) {
            if (ptr) *ptr = b.p;
            if (rows) *rows = b.r;
            if (cols) *cols = b.c;
            if (ld) *ld = b.ld;
            return 0;
        }
    return fail(VLSAT_EINVAL, std::string("unknown buffer ") + name);
}

// debug: synchronous strided copy of a named workspace buffer into dst (device, row pitch dst_ld floats)
int vlsat_debug_read(vlsat_plan p, const char* name, float* dst, int64_t dst_ld) {
    void* src = nullptr; int64_t rows = 0; int32_t cols = 0, ld = 0;
    int r = vlsat_debug_buffer(p, name, &src, &rows, &cols, &ld);
    if (r) return r;
    if (!dst || rows <= 0 || cols <= 0) return fail(VLSAT_EINVAL, "debug_read: nothing to copy");
    VLSAT_HIP_CHECK(hipDeviceSynchronize());
    VLSAT_HIP_CHECK(hipMemcpy2D(dst, (size_t)dst_ld * 4, src, (size_t)ld * 4, (size_t)cols * 4, (size_t)rows,
                                hipMemcpyDeviceToDevice));
    return 0;
}

}  // extern "C"
