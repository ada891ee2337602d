// The host-only part of a graph plan (engine_plan.hip adds the HIP objects: arena pool, staging, upload): the analysis of one (batch ids,
// edge list) -- scene runs, validation, CSR over sources, the attention tile tables and the three scheduling rules that shape them -- and
// the ONE list of the buffers of a plan's device arena, from which the layout, the carve, the two-stream budget and the debug table derive.
// No HIP header: tests/plan_graph_check.cpp compiles this with g++ against the code vlsat_plan_create had before.  Reached through
// engine.h, which states EvalScratch (two rows of the list) first.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vlsat.h"
#include "flash_pick.h"

namespace vlsat {

// Four ints of int4's size and alignment (asserted in engine_plan.hip; the tables reach the device as bytes).  An attention tile is
// (scene start, scene tokens, first query, head); a key range of the split-key mode is (first key tile, end key tile, part, -).
struct alignas(16) PlanTile { int x, y, z, w; };

// the query tiles of one (start, tokens) range: head, q-tile of `bq` queries (scene-major callers: consecutive ids share K/V -> same XCD)
inline void append_tile_rows(std::vector<PlanTile>& tiles, int64_t start, int64_t tokens, int heads, int bq) {
    for (int hh = 0; hh < heads; ++hh)
        for (int64_t q0 = 0; q0 < tokens; q0 += bq) tiles.push_back({(int)start, (int)tokens, (int)q0, hh});
}

// Many blocks (several rounds of the resident slots): the kernels map block b to tile xcd_remap(b) -- XCD b % 8 walks a
// contiguous range of tile ids in order -- and a scene's last query tile is usually mostly empty (1560 = 12 * 128 + 24:
// one wave of four has work).  Those light tiles go to the END of every XCD's range, so that the last, partly filled
// round of blocks is made of light work instead of ending on full tiles next to idle CUs.
inline void light_tiles_last(std::vector<PlanTile>& tiles) {
    if (tiles.size() < 2048) return;
    std::vector<PlanTile> full, part;
    for (const PlanTile& t : tiles) (t.z + FLASH_BQ <= t.y ? full : part).push_back(t);
    if (part.empty() || full.empty()) return;
    const size_t n = tiles.size(), q = n / 8, r = n % 8;
    std::vector<PlanTile> out;
    out.reserve(n);
    size_t fi = 0, pi = 0;
    for (size_t x = 0; x < 8; ++x) {
        const size_t cnt = q + (x < r ? 1 : 0);
        size_t np = part.size() * (x + 1) / 8 - part.size() * x / 8;          // this XCD's share of the light tiles
        np = std::min(np, cnt);
        size_t nf = std::min(cnt - np, full.size() - fi);
        np = cnt - nf;                                                          // (whatever the full list cannot cover)
        for (size_t i = 0; i < nf; ++i) out.push_back(full[fi++]);
        for (size_t i = 0; i < np && pi < part.size(); ++i) out.push_back(part[pi++]);
    }
    while (fi < full.size()) out.push_back(full[fi++]);                         // (rounding leftovers, if any)
    while (pi < part.size()) out.push_back(part[pi++]);
    if (out.size() == n) tiles.swap(out);
}

// Few blocks (one scene alone: ceil(T/128)*8 ~ 100 for 256 CUs): cut every block's key range into `parts`
// pieces so that about two rounds of 512 resident blocks exist; each piece keeps at least two key tiles.
// -> parts; above 1, every tile is there `parts` times and krange has its key range at the same index.
inline int split_keys(std::vector<PlanTile>& tiles, std::vector<PlanTile>& krange) {
    if (tiles.empty() || tiles.size() >= 512) return 1;
    const int parts = (int)std::min<size_t>(16, 1024 / tiles.size());
    if (parts <= 1) return 1;
    std::vector<PlanTile> split;
    for (const PlanTile& t : tiles) {
        const int kt = (t.y + 31) / 32;
        const int ps = std::max(1, std::min(parts, kt / 2));          // parts actually used by this scene
        for (int q = 0; q < parts; ++q) {
            split.push_back(t);
            const int a = q < ps ? (int)((int64_t)kt * q / ps) : 0, b = q < ps ? (int)((int64_t)kt * (q + 1) / ps) : 0;
            krange.push_back({a, b, q, 0});
        }
    }
    tiles.swap(split);
    return parts;
}

// Scenes of thousands of edges (cfg 5: one of 39 800): 256 queries per block share every K / V tile -- half the L2 -> LDS bytes
// per query, and the partly filled last tile is < 1/16 of a scene.  Built only when EVERY scene is that large (one table, one
// block size per launch), no keys are split and the K|V tensor is addressable with 32 bits; the forward uses it for half rows at
// head dim 64 (engine_forward.hip).
inline std::vector<PlanTile> big_tiles(const std::vector<int64_t>& edge_ptr, int64_t E, int H, int D, int big_min) {
    std::vector<PlanTile> big;
    if (E <= 0 || E * (int64_t)(2 * D) * 4 >= (int64_t)1 << 32) return big;
    int64_t min_t = INT64_MAX;
    for (size_t s = 0; s + 1 < edge_ptr.size(); ++s) { const int64_t T = edge_ptr[s + 1] - edge_ptr[s]; if (T > 0) min_t = std::min(min_t, T); }
    if (min_t >= big_min && min_t != INT64_MAX)
        for (size_t s = 0; s + 1 < edge_ptr.size(); ++s) append_tile_rows(big, edge_ptr[s], edge_ptr[s + 1] - edge_ptr[s], H, FLASH_BQ_BIG);
    if (big.size() < 1024) big.clear();          // (two rounds of the 512 resident blocks, as for the key split above)
    return big;
}

struct PlanCfg {                            // the handle values that plan creation reads
    int H = 8, D = 512, A = 256, edge_scope = 0, fa_split = 1, flash_bq_big_min = 4096, dual_stream = 2;
    int n_layers = 2, n_obj_class = 160, n_rel_class = 26, feature_transform = 0;
};

struct PlanGraph {
    int code = 0;                           // a refused graph: VLSAT_* and the text for vlsat_last_error (nothing else is valid then)
    std::string error;
    int S = 0, max_n = 0, max_e = 0, is_fc = 0, fa_parts = 1;
    std::vector<int32_t> node_ptr, src, dst, order, rowptr, edge_ptr32;    // [S+1], 3 x [max(E, 1)] (order: edges by source, stable), [N+1], [S+1]
    std::vector<int64_t> edge_ptr, bias_ptr;                               // [S+1], [S]: scene s has H n_s^2 bias values from bias_ptr[s]
    int64_t bias_total = 0;
    std::vector<PlanTile> tiles, krange, tiles_big;
    double flash_flops = 0;
};

inline PlanGraph plan_graph_analyse(const int64_t* bid, const int64_t* edges, int64_t N, int64_t E, const PlanCfg& c) {
    PlanGraph g;
    auto refuse = [&g](int code, const char* msg) { g.code = code; g.error = msg; return std::move(g); };
    // ---- scenes: maximal runs of equal batch id (must not re-appear) ----
    std::vector<int32_t> node_scene(N);
    g.node_ptr.push_back(0);
    {
        std::map<int64_t, int> seen;
        for (int64_t i = 0; i < N; ++i) {
            if (i == 0 || bid[i] != bid[i - 1]) {
                if (seen.count(bid[i])) return refuse(VLSAT_EINVAL, "batch_ids: nodes of a scene must be contiguous");
                seen[bid[i]] = 1;
                if (i) g.node_ptr.push_back((int32_t)i);
            }
            node_scene[i] = (int32_t)g.node_ptr.size() - 1;
        }
        g.node_ptr.push_back((int32_t)N);
    }
    g.S = (int)g.node_ptr.size() - 1;
    // ---- edges: same-scene endpoints, grouped by scene in node order ----
    const size_t Es = (size_t)std::max<int64_t>(E, 1);
    g.src.resize(Es); g.dst.resize(Es);
    g.edge_ptr.assign(g.S + 1, 0);
    int cur = 0;
    bool sorted_by_src = true;
    for (int64_t e = 0; e < E; ++e) {
        const int64_t a = edges[e], b = edges[E + e];
        if (a < 0 || a >= N || b < 0 || b >= N) return refuse(VLSAT_EINVAL, "edge index out of range");
        const int sa = node_scene[a];
        if (sa != node_scene[b]) return refuse(VLSAT_EINVAL, "edge joins nodes of different scenes");
        if (sa < cur) return refuse(VLSAT_EGRAPH, "edges are not grouped by scene in node order");
        while (cur < sa) g.edge_ptr[++cur] = e;
        g.src[e] = (int32_t)a; g.dst[e] = (int32_t)b;
        if (e && g.src[e] < g.src[e - 1]) sorted_by_src = false;
    }
    while (cur < g.S) g.edge_ptr[++cur] = E;
    // ---- CSR over sources (stable counting sort) ----
    g.rowptr.assign(N + 1, 0); g.order.resize(Es);
    for (int64_t e = 0; e < E; ++e) g.rowptr[g.src[e] + 1]++;
    for (int64_t i = 0; i < N; ++i) g.rowptr[i + 1] += g.rowptr[i];
    {
        std::vector<int32_t> fill(g.rowptr.begin(), g.rowptr.end() - 1);
        for (int64_t e = 0; e < E; ++e) g.order[fill[g.src[e]]++] = (int32_t)e;
    }
    // ---- per scene: sizes, fully connected or not, bias offset; flash tiles: scene-major, head, q-tile ----
    g.is_fc = sorted_by_src;
    g.bias_ptr.resize(g.S);
    g.edge_ptr32.assign(g.edge_ptr.begin(), g.edge_ptr.end());
    if (c.edge_scope == 1) { g.edge_ptr32.assign((size_t)g.S + 1, (int32_t)E); g.edge_ptr32[0] = 0; }   // one range: the whole batch
    if (c.edge_scope == 1 && E > 0) {       // reference multi-scene call: one attention over all edges
        append_tile_rows(g.tiles, 0, E, c.H, FLASH_BQ);
        g.flash_flops += 4.0 * (double)E * (double)E * c.D;
    }
    for (int s = 0; s < g.S; ++s) {
        const int64_t T = g.edge_ptr[s + 1] - g.edge_ptr[s], n = g.node_ptr[s + 1] - g.node_ptr[s];
        g.max_n = std::max(g.max_n, (int)n); g.max_e = std::max(g.max_e, (int)T);
        if (T != n * (n - 1)) g.is_fc = 0;
        if (c.edge_scope == 0) {
            append_tile_rows(g.tiles, g.edge_ptr[s], T, c.H, FLASH_BQ);
            g.flash_flops += 4.0 * (double)T * (double)T * c.D;
        }
        g.bias_ptr[s] = g.bias_total;
        g.bias_total += (int64_t)c.H * n * n;
    }
    light_tiles_last(g.tiles);
    if (c.fa_split) g.fa_parts = split_keys(g.tiles, g.krange);
    if (c.edge_scope == 0 && g.fa_parts <= 1) g.tiles_big = big_tiles(g.edge_ptr, E, c.H, c.D, c.flash_bq_big_min);
    return g;
}

// ---- the workspace: one device arena carved into every buffer of a plan ----

struct WsParams {
    size_t Ns, Es, S, bias_total, n_tiles, n_tiles_big;      // N, max(E, 1) (the rows of node / edge buffers), scenes, table lengths
    size_t H, LDX, NPC, A, layers, C, R, P;                  // LDX, NPC: ldx_of, npc_of (engine.h)
    int fa_parts;
    bool feature_transform, dual;
    size_t kvx_slots() const { return dual ? std::max<size_t>(1, layers) : 1; }      // two-stream plans keep one K|V projection of X3 per layer
    // MODEL.feature_transform: point rows R = N*P (objects) or E (relation encoders, P = 1), one phase at a time:
    //   rows [R,64] h1, [R,64], [R,128], [R,1024] STN convs (the last two double as conv2/conv3 of the main chain),
    //   [R,64] h1';  per object: 1024 + 512 + 256 + 4096
    size_t stn_floats() const { return std::max(Ns * P, Es) * (64 + 64 + 128 + 1024 + 64) + std::max(Ns, Es) * (1024 + 512 + 256 + 4096); }
};
// `dual` here is the wish: launch-bound plans (every edge GEMM fits one round of the grid; dual_stream = 2: every plan) run the 2D twin
// stages on a second stream and carry a second scratch set for them -- unless that takes the plan past the budget (ws_layout)
inline WsParams ws_params(const PlanCfg& c, const PlanGraph& g, int64_t N, int64_t E, int P) {
    return {(size_t)N, (size_t)std::max<int64_t>(E, 1), (size_t)g.S, (size_t)g.bias_total, g.tiles.size(), g.tiles_big.size(),
            (size_t)c.H, (size_t)(c.D + c.A), (size_t)(6 * c.D + c.A), (size_t)c.A, (size_t)c.n_layers, (size_t)c.n_obj_class, (size_t)c.n_rel_class, (size_t)P,
            g.fa_parts, c.feature_transform != 0, c.dual_stream && E > 0 && (c.dual_stream > 1 || E <= 8192)};
}
// a plan whose workspace would exceed this with the second scratch set of the two-stream mode runs on one stream
constexpr size_t DUAL_WS_BUDGET = size_t(48) << 30;

// X(member of vlsat_plan_s, element type, rows, elements per row, in which plans it exists, columns vlsat_debug_buffer shows or -1); rows and
// the two expressions are in terms of the WsParams w.  In arena order: the index tables first, in the order they are packed into the staging
// buffer, then the work buffers from F on -- node rows | bias, edge rows | node cross-attention rows, evaluation scratch (0.6 KB per edge,
// 2.6 KB per node; its layout: engine.h EvalScratch) | the second scratch set of two-stream plans | KVx, feature-transform scratch, split-key
// partials.  The two-stream budget counts everything up to and including KVx: what only a two-stream plan has stays in front of it.
enum WsRows { WS_NODES, WS_NODES1, WS_EDGES, WS_SCENES, WS_SCENES1, WS_FLAT };      // N, N + 1, max(E, 1), S, S + 1, one row
#define VLSAT_WS_BUFFERS(X)                                                                                                                      \
    X(d_src, int32_t, WS_EDGES, 1, true, -1) X(d_dst, int32_t, WS_EDGES, 1, true, -1) X(d_order, int32_t, WS_EDGES, 1, true, -1)                 \
    X(d_rowptr, int32_t, WS_NODES1, 1, true, -1) X(d_scene_ptr, int32_t, WS_SCENES1, 1, true, -1) X(d_bias_ptr, int64_t, WS_SCENES, 1, true, -1) \
    X(d_edge_ptr32, int32_t, WS_SCENES1, 1, true, -1) X(d_tiles, PlanTile, WS_FLAT, std::max<size_t>(w.n_tiles, 1), true, -1)                    \
    X(d_krange, PlanTile, WS_FLAT, w.n_tiles, w.fa_parts > 1, -1) X(d_tiles_big, PlanTile, WS_FLAT, w.n_tiles_big, w.n_tiles_big > 0, -1)        \
    X(F, float, WS_NODES, 768, true, 768) X(X3, float, WS_NODES, w.LDX, true, 512) X(X2, float, WS_NODES, w.LDX, true, 512)                      \
    X(NP, float, WS_NODES, w.NPC, true, (int)w.NPC) X(QKVn, float, WS_NODES, 1536, true, -1) X(On, float, WS_NODES, 512, true, 512)              \
    X(T256, float, WS_NODES, 256, true, -1) X(T768, float, WS_NODES, w.LDX, true, -1) X(rs, float, WS_NODES, 1, true, -1)                        \
    X(bias, float, WS_FLAT, std::max<size_t>(w.bias_total, 1), true, 0)                                                                          \
    X(H1, float, WS_EDGES, 128, true, 128) X(H2, float, WS_EDGES, 128, true, -1) X(E3, float, WS_EDGES, 512, true, 512)                          \
    X(E2, float, WS_EDGES, 512, true, 512) X(Hbig, float, WS_EDGES, 1024, true, 1024) X(KP, float, WS_EDGES, 512, true, 512)                     \
    X(G, float, WS_EDGES, w.A, true, (int)w.A) X(Qe, float, WS_EDGES, 512, true, 512) X(KVe, float, WS_EDGES, 1024, true, 1024)                  \
    X(Oe, float, WS_EDGES, 512, true, 512) X(Q2n, float, WS_NODES, 512, true, -1) X(On2, float, WS_NODES, 512, true, -1)                         \
    X(ev_f, float, WS_FLAT, eval_scratch_floats(w.Ns, w.Es, w.C, w.R), true, -1) X(ev_i, int32_t, WS_FLAT, eval_scratch_ints(w.Ns, w.Es, w.R), true, -1) \
    X(NP2, float, WS_NODES, w.NPC, w.dual, -1) X(Hbig2, float, WS_EDGES, 1024, w.dual, -1) X(KP2, float, WS_EDGES, 512, w.dual, -1)              \
    X(G2, float, WS_EDGES, w.A, w.dual, -1) X(T768b, float, WS_NODES, w.LDX, w.dual, -1) X(rs2, float, WS_NODES, 1, w.dual, -1)                  \
    X(H2b, float, WS_EDGES, 128, w.dual, -1) X(KVe2, float, WS_EDGES, 1024, w.dual, -1)                                                          \
    X(KVx, float, WS_NODES, 1024 * w.kvx_slots(), true, -1) X(stn_ws, float, WS_FLAT, w.stn_floats(), w.feature_transform, -1)                   \
    X(fa_opart, float, WS_EDGES, w.fa_parts * 512, w.fa_parts > 1, -1) X(fa_m, float, WS_EDGES, w.fa_parts * w.H, w.fa_parts > 1, -1)            \
    X(fa_l, float, WS_EDGES, w.fa_parts * w.H, w.fa_parts > 1, -1)
// X(member, the buffer it is a view of, first element): the relation-head hidden layers re-use the nn_edge hidden buffer
#define VLSAT_WS_VIEWS(X) X(R1, Hbig, 0) X(R2, Hbig, w.Es * 512)

#define VLSAT_WS_ID(m, T, rows, per, when, cols) WS_##m,
enum WsId { VLSAT_WS_BUFFERS(VLSAT_WS_ID) WS_COUNT, WS_INDEX_END = WS_F, WS_DUAL_BUDGET_END = WS_KVx + 1 };
#undef VLSAT_WS_ID

inline size_t ws_rows(WsRows r, const WsParams& w) {
    return r == WS_NODES ? w.Ns : r == WS_NODES1 ? w.Ns + 1 : r == WS_EDGES ? w.Es : r == WS_SCENES ? w.S : r == WS_SCENES1 ? w.S + 1 : 1;
}

struct WsLayout {
    WsParams w;                             // as given, except `dual`: whether the plan IS a two-stream plan
    size_t off[WS_COUNT], bytes[WS_COUNT];  // bytes 0: not in this plan
    size_t total, index_bytes;              // every buffer padded to 256 bytes; index_bytes: the index tables, which one upload fills
    int n_index;                            // how many index tables there are
};

inline WsLayout ws_layout(const WsParams& params) {
    WsLayout L{params, {}, {}, 0, 0, 0};
    const WsParams& w = L.w;
    auto sizes = [&] {
#define VLSAT_WS_SIZE(m, T, rows, per, when, cols) L.bytes[WS_##m] = (when) ? ws_rows(rows, w) * (size_t)(per) * sizeof(T) : 0;
        VLSAT_WS_BUFFERS(VLSAT_WS_SIZE)
#undef VLSAT_WS_SIZE
    };
    sizes();
    if (w.dual) {                           // ... unless the second scratch set (KVx at a slot per layer) would take the plan past the budget
        size_t need = 0;
        for (int id = 0; id < WS_DUAL_BUDGET_END; ++id) need += L.bytes[id];
        if (need > DUAL_WS_BUDGET) { L.w.dual = false; sizes(); }
    }
    for (int id = 0; id < WS_COUNT; ++id) {
        if (id == WS_INDEX_END) L.index_bytes = L.total;
        L.off[id] = L.total;
        L.total += (L.bytes[id] + 255) & ~size_t(255);
        L.n_index += id < WS_INDEX_END && L.bytes[id];
    }
    return L;
}

// every buffer of the list at its offset in the arena (nullptr: not in this plan), and the views; Plan: vlsat_plan_s
template <class Plan>
inline void ws_carve(Plan* p, char* arena, const WsLayout& L) {
    const WsParams& w = L.w;
#define VLSAT_WS_CARVE(m, T, rows, per, when, cols)                                                   \
    static_assert(sizeof(*p->m) == sizeof(T) && alignof(decltype(*p->m)) == alignof(T), #m);          \
    p->m = L.bytes[WS_##m] ? reinterpret_cast<decltype(p->m)>(arena + L.off[WS_##m]) : nullptr;
    VLSAT_WS_BUFFERS(VLSAT_WS_CARVE)
#undef VLSAT_WS_CARVE
#define VLSAT_WS_VIEW(m, of, first) p->m = p->of + (first);
    VLSAT_WS_VIEWS(VLSAT_WS_VIEW)
#undef VLSAT_WS_VIEW
}

// the index tables of `g`, each at its offset, into a staging buffer of L.index_bytes (the padding between them is left as it is)
inline void pack_index_tables(const PlanGraph& g, const WsLayout& L, char* staging) {
    const void* host[] = {g.src.data(), g.dst.data(), g.order.data(), g.rowptr.data(), g.node_ptr.data(), g.bias_ptr.data(), g.edge_ptr32.data(),
                          g.tiles.empty() ? nullptr : g.tiles.data(), g.krange.data(), g.tiles_big.data()};      // in the list's order
    static_assert(sizeof host / sizeof host[0] == WS_INDEX_END, "one host table per index buffer");
    for (int id = 0; id < WS_INDEX_END; ++id)
        if (L.bytes[id] && host[id]) memcpy(staging + L.off[id], host[id], L.bytes[id]);
}

// A fresh arena has the next SIZE CLASS (2^k or 1.5 * 2^k bytes: 1, 1.5, 2, 3, 4, 6, ... MiB): an evaluation loop sees a new graph size
// almost every scene, and with exact sizes nearly every plan would allocate and nearly every evicted one would end in hipFree (which waits
// for the device: profiles/r02_hip_api_trace.txt had 48 of them in 80 forwards before the classes)
inline size_t arena_size_class(size_t total) {
    size_t cls = size_t(1) << 20;
    while (cls < total) cls = (cls & (cls - 1)) ? (cls / 3) * 4 : cls + cls / 2;
    return cls;
}
// the smallest pooled arena that fits (and is not absurdly larger), or -1; Pool: a sequence of things with `.bytes`
template <class Pool>
inline int arena_pool_pick(const Pool& pool, size_t total) {
    int best = -1;
    for (size_t i = 0; i < pool.size(); ++i)
        if (pool[i].bytes >= total && pool[i].bytes <= 4 * total + (64u << 20) && (best < 0 || pool[i].bytes < pool[best].bytes)) best = (int)i;
    return best;
}

}  // namespace vlsat
