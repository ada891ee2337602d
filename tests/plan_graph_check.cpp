// Host-only check of csrc/plan_graph.h (built with g++ by tests/host_check.py; opens no device): the graph analysis, the workspace list and
// the arena arithmetic against the body vlsat_plan_create had before them, kept here word for word from the scene loop down to the offset
// loop (legacy_plan_create; `int4` is the header's four-int tile, `fail` records code and text, the arena pick is a function of its own
// because the old one sat between HIP calls, and the list of items is handed out at the end).  Old and new must agree with NO difference in
// every index table (compared as the packed staging buffer, byte for byte), S, max_n, max_e, is_fc, fa_parts, the tile counts, flash_flops
// (bit-equal), bias_total, every buffer's existence, offset and size, R1 / R2, total, index_bytes, the two-stream decision, kvx_slots,
// stn_ws_floats and, for refused graphs, code and text.  Prints one "<group> -> ok ..." line per group and "ws | <case> | <bytes>" for the
// three graphs of tests/plan_cases.py; exits 1 at the first difference.  With the argument "time" it times plan creation instead.
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <cstring>
#include <memory>

#define VLSAT_EVAL_SCRATCH_ONLY
#include "engine.h"

using namespace vlsat;

// ---- what the old body needs around it ----
typedef PlanTile int4;
static int4 make_int4(int x, int y, int z, int w) { return {x, y, z, w}; }
static int g_code = 0;
static std::string g_text;
static int fail(int code, const std::string& msg) { g_code = code; g_text = msg; return code; }
struct Dims { int n_layers = 2, n_obj_class = 160, n_rel_class = 26, feature_transform = 0; };
struct Ctx {
    Dims d;
    int dual_stream = 2, fa_split = 1, edge_scope = 0, D = 512, A = 256, H = 8, flash_bq_big_min = 4096;
};
static int ldx_of(const Ctx* h) { return h->D + h->A; }
static int npc_of(const Ctx* h) { return 6 * h->D + h->A; }
struct Staging { char* p = nullptr; };
struct Plan {                               // the members of vlsat_plan_s that plan creation sets
    Ctx* h = nullptr;
    int64_t N = 0, E = 0;
    int P = 0, S = 0, max_n = 0, is_fc = 0;
    std::vector<int32_t> node_ptr;
    std::vector<int64_t> edge_ptr;
    size_t ws_bytes = 0;
    char* arena = nullptr;
    int32_t *d_src = nullptr, *d_dst = nullptr, *d_rowptr = nullptr, *d_order = nullptr, *d_scene_ptr = nullptr, *d_edge_ptr32 = nullptr;
    int max_e = 0;
    int64_t* d_bias_ptr = nullptr;
    int4 *d_tiles = nullptr, *d_tiles_big = nullptr, *d_krange = nullptr;
    int n_tiles = 0, n_tiles_big = 0, fa_parts = 1;
    float *fa_opart = nullptr, *fa_m = nullptr, *fa_l = nullptr;
    double flash_flops = 0;
    float *F = nullptr, *X3 = nullptr, *X2 = nullptr, *NP = nullptr, *QKVn = nullptr, *On = nullptr, *T256 = nullptr, *T768 = nullptr, *rs = nullptr, *bias = nullptr;
    float *H1 = nullptr, *H2 = nullptr, *E3 = nullptr, *E2 = nullptr, *Hbig = nullptr, *KP = nullptr, *G = nullptr, *Qe = nullptr, *KVe = nullptr, *Oe = nullptr;
    float *R1 = nullptr, *R2 = nullptr, *prob = nullptr, *stn_ws = nullptr;
    size_t stn_ws_floats = 0;
    bool dual = false;
    float *NP2 = nullptr, *Hbig2 = nullptr, *KP2 = nullptr, *G2 = nullptr, *T768b = nullptr, *rs2 = nullptr, *H2b = nullptr;
    float *Q2n = nullptr, *On2 = nullptr, *KVx = nullptr, *ev_f = nullptr, *KVe2 = nullptr;
    int kvx_slots = 1;
    int32_t* ev_i = nullptr;
};
struct Arena { char* p = nullptr; size_t bytes = 0; };
struct OldItem { void** dst; size_t bytes; };

// p->arena is set by the caller (the old code took it from the pool or from hipMalloc between the size loop and the offset loop), st->p
// is a buffer of at least the index tables' bytes
static int legacy_plan_create(Ctx* h, const int64_t* bid, const int64_t* edges, int64_t N, int64_t E, int32_t P, Plan* p, Staging* st,
                              std::vector<OldItem>* items_out, size_t* index_bytes_out) {
    p->h = h; p->N = N; p->E = E; p->P = P;
    const int H = h->H, D = h->D;
    const size_t LDX = (size_t)ldx_of(h), NPC = (size_t)npc_of(h), A = (size_t)h->A;
    // ---- scenes: maximal runs of equal batch id (must not re-appear) ----
    std::vector<int32_t> node_scene(N);
    p->node_ptr.push_back(0);
    {
        std::map<int64_t, int> seen;
        for (int64_t i = 0; i < N; ++i) {
            if (i == 0 || bid[i] != bid[i - 1]) {
                if (seen.count(bid[i])) return fail(VLSAT_EINVAL, "batch_ids: nodes of a scene must be contiguous");
                seen[bid[i]] = 1;
                if (i) p->node_ptr.push_back((int32_t)i);
            }
            node_scene[i] = (int32_t)p->node_ptr.size() - 1;
        }
        p->node_ptr.push_back((int32_t)N);
    }
    p->S = (int)p->node_ptr.size() - 1;
    for (int s = 0; s < p->S; ++s) p->max_n = std::max(p->max_n, p->node_ptr[s + 1] - p->node_ptr[s]);
    // ---- edges: same-scene endpoints, grouped by scene in node order ----
    const size_t Es = (size_t)std::max<int64_t>(E, 1), Ns = (size_t)N;
    std::vector<int32_t> src(Es), dst(Es);
    p->edge_ptr.assign(p->S + 1, 0);
    int cur = 0;
    bool sorted_by_src = true;
    for (int64_t e = 0; e < E; ++e) {
        const int64_t a = edges[e], b = edges[E + e];
        if (a < 0 || a >= N || b < 0 || b >= N) return fail(VLSAT_EINVAL, "edge index out of range");
        const int sa = node_scene[a];
        if (sa != node_scene[b]) return fail(VLSAT_EINVAL, "edge joins nodes of different scenes");
        if (sa < cur) return fail(VLSAT_EGRAPH, "edges are not grouped by scene in node order");
        while (cur < sa) p->edge_ptr[++cur] = e;
        src[e] = (int32_t)a; dst[e] = (int32_t)b;
        if (e && src[e] < src[e - 1]) sorted_by_src = false;
    }
    while (cur < p->S) p->edge_ptr[++cur] = E;
    // ---- CSR over sources (stable counting sort) ----
    std::vector<int32_t> rowptr(N + 1, 0), order(Es);
    for (int64_t e = 0; e < E; ++e) rowptr[src[e] + 1]++;
    for (int64_t i = 0; i < N; ++i) rowptr[i + 1] += rowptr[i];
    {
        std::vector<int32_t> fill(rowptr.begin(), rowptr.end() - 1);
        for (int64_t e = 0; e < E; ++e) order[fill[src[e]]++] = (int32_t)e;
    }
    p->is_fc = sorted_by_src;
    for (int s = 0; s < p->S && p->is_fc; ++s) {
        const int64_t n = p->node_ptr[s + 1] - p->node_ptr[s];
        if (p->edge_ptr[s + 1] - p->edge_ptr[s] != n * (n - 1)) p->is_fc = 0;
    }
    // ---- flash tiles: scene-major, head, q-tile (consecutive ids share K/V -> same XCD) ----
    std::vector<int4> tiles;
    std::vector<int64_t> bias_ptr(p->S);
    int64_t bias_total = 0;
    if (h->edge_scope == 1 && E > 0) {       // reference multi-scene call: one attention over all edges
        for (int hh = 0; hh < H; ++hh)
            for (int64_t q0 = 0; q0 < E; q0 += FLASH_BQ) tiles.push_back(make_int4(0, (int)E, (int)q0, hh));
        p->flash_flops += 4.0 * (double)E * (double)E * D;
    }
    for (int s = 0; s < p->S; ++s) {
        const int64_t T = p->edge_ptr[s + 1] - p->edge_ptr[s];
        if (h->edge_scope == 0) {
            for (int hh = 0; hh < H; ++hh)
                for (int64_t q0 = 0; q0 < T; q0 += FLASH_BQ)
                    tiles.push_back(make_int4((int)p->edge_ptr[s], (int)T, (int)q0, hh));
            p->flash_flops += 4.0 * (double)T * (double)T * D;
        }
        const int64_t n = p->node_ptr[s + 1] - p->node_ptr[s];
        bias_ptr[s] = bias_total;
        bias_total += (int64_t)H * n * n;
    }
    // Many blocks (several rounds of the resident slots): the kernels map block b to tile xcd_remap(b) -- XCD b % 8 walks a
    // contiguous range of tile ids in order -- and a scene's last query tile is usually mostly empty (1560 = 12 * 128 + 24:
    // one wave of four has work).  Those light tiles go to the END of every XCD's range, so that the last, partly filled
    // round of blocks is made of light work instead of ending on full tiles next to idle CUs.
    if (tiles.size() >= 2048) {
        std::vector<int4> full, part;
        for (const int4& t : tiles) (t.z + FLASH_BQ <= t.y ? full : part).push_back(t);
        if (!part.empty() && !full.empty()) {
            const size_t n = tiles.size(), q = n / 8, r = n % 8;
            std::vector<int4> out;
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
    }
    // Few blocks (one scene alone: ceil(T/128)*8 ~ 100 for 256 CUs): cut every block's key range into `parts`
    // pieces so that about two rounds of 512 resident blocks exist; each piece keeps at least two key tiles.
    std::vector<int4> krange;
    if (!tiles.empty() && tiles.size() < 512 && h->fa_split) {
        int parts = (int)std::min<size_t>(16, 1024 / tiles.size());
        if (parts > 1) {
            std::vector<int4> split;
            for (const int4& t : tiles) {
                const int kt = (t.y + 31) / 32;
                const int ps = std::max(1, std::min(parts, kt / 2));          // parts actually used by this scene
                for (int q = 0; q < parts; ++q) {
                    split.push_back(t);
                    const int a = q < ps ? (int)((int64_t)kt * q / ps) : 0, b = q < ps ? (int)((int64_t)kt * (q + 1) / ps) : 0;
                    krange.push_back(make_int4(a, b, q, 0));
                }
            }
            tiles.swap(split);
            p->fa_parts = parts;
        }
    }
    p->n_tiles = (int)tiles.size();
    // Scenes of thousands of edges (cfg 5: one of 39 800): 256 queries per block share every K / V tile -- half the L2 -> LDS bytes
    // per query, and the partly filled last tile is < 1/16 of a scene.  Built only when EVERY scene is that large (one table, one
    // block size per launch); the forward uses it for half rows at head dim 64 (engine_forward.hip).
    std::vector<int4> tiles_big;
    if (h->edge_scope == 0 && p->fa_parts <= 1 && E > 0 && E * (int64_t)(2 * D) * 4 < (int64_t)1 << 32) {
        int64_t min_t = INT64_MAX;
        for (int s = 0; s < p->S; ++s) { const int64_t T = p->edge_ptr[s + 1] - p->edge_ptr[s]; if (T > 0) min_t = std::min(min_t, T); }
        if (min_t >= h->flash_bq_big_min && min_t != INT64_MAX)
            for (int s = 0; s < p->S; ++s) {
                const int64_t T = p->edge_ptr[s + 1] - p->edge_ptr[s];
                for (int hh = 0; hh < H; ++hh)
                    for (int64_t q0 = 0; q0 < T; q0 += FLASH_BQ_BIG) tiles_big.push_back(make_int4((int)p->edge_ptr[s], (int)T, (int)q0, hh));
            }
        if (tiles_big.size() < 1024) tiles_big.clear();          // (two rounds of the 512 resident blocks, as for the key split above)
    }
    p->n_tiles_big = (int)tiles_big.size();
    // ---- one device arena; the index tables come first, in the order they are packed into the staging buffer ----
    struct Item { void** dst; size_t bytes; const void* host; };
    std::vector<Item> items;
    auto want = [&](auto** ptr, size_t count, const void* host = nullptr) {
        items.push_back({reinterpret_cast<void**>(ptr), count * sizeof(**ptr), host});
    };
    want(&p->d_src, Es, src.data()); want(&p->d_dst, Es, dst.data()); want(&p->d_order, Es, order.data());
    want(&p->d_rowptr, Ns + 1, rowptr.data()); want(&p->d_scene_ptr, (size_t)p->S + 1, p->node_ptr.data());
    want(&p->d_bias_ptr, (size_t)p->S, bias_ptr.data());
    std::vector<int32_t> edge_ptr32(p->edge_ptr.begin(), p->edge_ptr.end());
    if (h->edge_scope == 1) { edge_ptr32.assign((size_t)p->S + 1, (int32_t)E); edge_ptr32[0] = 0; }   // one range: the whole batch
    for (int sc = 0; sc < p->S; ++sc) p->max_e = std::max<int>(p->max_e, (int)(p->edge_ptr[sc + 1] - p->edge_ptr[sc]));
    want(&p->d_edge_ptr32, (size_t)p->S + 1, edge_ptr32.data());
    want(&p->d_tiles, std::max<size_t>(tiles.size(), 1), tiles.empty() ? nullptr : tiles.data());
    if (p->fa_parts > 1) want(&p->d_krange, krange.size(), krange.data());
    if (!tiles_big.empty()) want(&p->d_tiles_big, tiles_big.size(), tiles_big.data());
    const size_t n_index_items = items.size();
    want(&p->F, Ns * 768); want(&p->X3, Ns * LDX); want(&p->X2, Ns * LDX); want(&p->NP, Ns * NPC);
    want(&p->QKVn, Ns * 1536); want(&p->On, Ns * 512); want(&p->T256, Ns * 256); want(&p->T768, Ns * LDX);
    want(&p->rs, Ns); want(&p->bias, (size_t)std::max<int64_t>(bias_total, 1));
    want(&p->H1, Es * 128); want(&p->H2, Es * 128); want(&p->E3, Es * 512); want(&p->E2, Es * 512);
    want(&p->Hbig, Es * 1024); want(&p->KP, Es * 512); want(&p->G, Es * A);
    want(&p->Qe, Es * 512); want(&p->KVe, Es * 1024); want(&p->Oe, Es * 512);
    want(&p->Q2n, Ns * 512); want(&p->On2, Ns * 512);
    {   // evaluation scratch (vlsat_process_val_counts): 0.6 KB per edge, 2.6 KB per node
        const size_t C = (size_t)h->d.n_obj_class, R = (size_t)h->d.n_rel_class;
        want(&p->ev_f, eval_scratch_floats(Ns, (size_t)E, C, R));      // (the layout: engine.h EvalScratch)
        want(&p->ev_i, eval_scratch_ints(Ns, (size_t)E, R));
    }
    // launch-bound plans (every edge GEMM fits one round of the grid): second scratch set for the 2D twin stages
    p->dual = h->dual_stream && E > 0 && (h->dual_stream > 1 || E <= 8192);      // (dual_stream = 2: every plan)
    if (p->dual) {                         // ... unless the second scratch set would take the plan past the budget
        size_t base = 0;
        for (auto& it : items) base += it.bytes;
        const size_t extra = (Ns * (size_t)(NPC + LDX + 1 + 1024 * (size_t)h->d.n_layers) + Es * (size_t)(1024 + 512 + A + 128 + 1024)) * sizeof(float);
        if (base + extra > DUAL_WS_BUDGET) p->dual = false;
    }
    if (p->dual) {
        want(&p->NP2, Ns * NPC); want(&p->Hbig2, Es * 1024); want(&p->KP2, Es * 512); want(&p->G2, Es * A);
        want(&p->T768b, Ns * LDX); want(&p->rs2, Ns); want(&p->H2b, Es * 128);
        want(&p->KVe2, Es * 1024);
        p->kvx_slots = std::max(1, (int)h->d.n_layers);
    }
    want(&p->KVx, Ns * 1024 * (size_t)p->kvx_slots);
    if (h->d.feature_transform) {
        // point rows R = N*P (objects) or E (relation encoders, P = 1), one phase at a time:
        //   rows [R,64] h1, [R,64], [R,128], [R,1024] STN convs (the last two double as conv2/conv3 of the main chain),
        //   [R,64] h1';  per object: 1024 + 512 + 256 + 4096
        const size_t R = std::max<size_t>(Ns * (size_t)P, Es), O = std::max(Ns, Es);
        p->stn_ws_floats = R * (64 + 64 + 128 + 1024 + 64) + O * (1024 + 512 + 256 + 4096);
        want(&p->stn_ws, p->stn_ws_floats);
    }
    if (p->fa_parts > 1) {
        want(&p->fa_opart, (size_t)p->fa_parts * Es * 512);
        want(&p->fa_m, (size_t)p->fa_parts * Es * H); want(&p->fa_l, (size_t)p->fa_parts * Es * H);
    }
    auto pad = [](size_t b) { return (b + 255) & ~size_t(255); };
    size_t total = 0, index_bytes = 0;
    for (size_t i = 0; i < items.size(); ++i) {
        total += pad(items[i].bytes);
        if (i + 1 == n_index_items) index_bytes = total;
    }
    size_t off = 0;
    for (auto& it : items) {
        *it.dst = p->arena + off;
        off += pad(it.bytes);
    }
    p->R1 = p->Hbig;                 // relation-head hidden layers re-use the nn_edge hidden buffer
    p->R2 = p->Hbig + Es * 512;
    p->prob = nullptr;
    p->ws_bytes = total;
    off = 0;
    for (size_t i = 0; i < n_index_items; ++i) {
        if (items[i].host) std::memcpy(st->p + off, items[i].host, items[i].bytes);
        off += pad(items[i].bytes);
    }
    for (auto& it : items) items_out->push_back({it.dst, it.bytes});      // (not in the old body: what the comparison reads)
    *index_bytes_out = index_bytes;
    return 0;
}

// the old pick from the pool and the old size class
static void legacy_arena(const std::vector<Arena>& arena_pool, size_t total, int* best_out, size_t* cls_out) {
    int best = -1;
    for (size_t i = 0; i < arena_pool.size(); ++i)
        if (arena_pool[i].bytes >= total && arena_pool[i].bytes <= 4 * total + (64u << 20) &&
            (best < 0 || arena_pool[i].bytes < arena_pool[best].bytes))
            best = (int)i;
    size_t cls = size_t(1) << 20;
    while (cls < total) cls = (cls & (cls - 1)) ? (cls / 3) * 4 : cls + cls / 2;      // 1, 1.5, 2, 3, 4, 6, ... MiB
    *best_out = best; *cls_out = cls;
}

// ---- graphs ----
struct Graph {
    std::string name;
    std::vector<int64_t> bid, src, dst;
    std::vector<int64_t> edges() const { std::vector<int64_t> e(src); e.insert(e.end(), dst.begin(), dst.end()); return e; }
    int64_t N() const { return (int64_t)bid.size(); }
    int64_t E() const { return (int64_t)src.size(); }
};
// one more scene of n nodes: fully connected, source-major (t < 0), or with t edges, sorted by source, from node i to i + 1 + k (mod n)
static void add_scene(Graph& g, int n, int64_t t = -1) {
    const int64_t base = g.N(), id = g.bid.empty() ? 0 : g.bid.back() + 1;
    for (int i = 0; i < n; ++i) g.bid.push_back(id);
    if (t < 0) {
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) if (a != b) { g.src.push_back(base + a); g.dst.push_back(base + b); }
    } else {
        for (int64_t e = 0; e < t; ++e) {
            const int64_t a = e * n / t;
            g.src.push_back(base + a); g.dst.push_back(base + (a + 1 + e % std::max(1, n - 1)) % n);
        }
    }
}
static Graph fc(const std::string& name, std::initializer_list<int> sizes) {
    Graph g; g.name = name;
    for (int n : sizes) add_scene(g, n);
    return g;
}
static Graph repeat(const std::string& name, int scenes, int n, int64_t t = -1) {
    Graph g; g.name = name;
    for (int s = 0; s < scenes; ++s) add_scene(g, n, t);
    return g;
}

// ---- the comparison ----
static long g_cases = 0;
[[noreturn]] static void differ(const std::string& what, const std::string& where, long long a = 0, long long b = 0) {
    printf("%s -> FAILED at %s (old %lld, new %lld)\n", what.c_str(), where.c_str(), a, b);
    exit(1);
}
static Ctx ctx_of(const PlanCfg& c) {
    Ctx h;
    h.d.n_layers = c.n_layers; h.d.n_obj_class = c.n_obj_class; h.d.n_rel_class = c.n_rel_class; h.d.feature_transform = c.feature_transform;
    h.dual_stream = c.dual_stream; h.fa_split = c.fa_split; h.edge_scope = c.edge_scope; h.D = c.D; h.A = c.A; h.H = c.H; h.flash_bq_big_min = c.flash_bq_big_min;
    return h;
}
static std::string cfg_text(const PlanCfg& c, int P) {
    char b[160];
    snprintf(b, sizeof b, " [H %d scope %d split %d dual %d ft %d layers %d bigmin %d P %d]", c.H, c.edge_scope, c.fa_split, c.dual_stream, c.feature_transform,
             c.n_layers, c.flash_bq_big_min, P);
    return b;
}
static char* const FAKE_ARENA = reinterpret_cast<char*>(uintptr_t(1) << 32);      // offsets only: never dereferenced

struct Outcome { int code; size_t total; int dual, fa_parts, n_tiles, n_tiles_big, is_fc, S; };

// old and new on one graph and one configuration; real_arena: carve a host buffer of exactly `total` bytes and write every region
static Outcome compare(const Graph& gr, const PlanCfg& c, int P, bool real_arena = false) {
    const std::string what = gr.name + cfg_text(c, P);
    const std::vector<int64_t> ed = gr.edges();
    const int64_t N = gr.N(), E = gr.E();
    const int64_t* edges = E ? ed.data() : nullptr;
    ++g_cases;
    // new
    PlanGraph g = plan_graph_analyse(gr.bid.data(), edges, N, E, c);
    // old
    Ctx h = ctx_of(c);
    Plan op;
    std::vector<OldItem> items;
    size_t old_index_bytes = 0;
    std::vector<char> old_stage((size_t)(N + 3 * std::max<int64_t>(E, 1)) * 4 + 4096 + (size_t)(g.tiles.size() * 3 + g.tiles_big.size() + 2 * g.S + 64) * 16 + 12 * 256, 0);
    Staging st{old_stage.data()};
    op.arena = FAKE_ARENA;
    g_code = 0; g_text.clear();
    const int rc = legacy_plan_create(&h, gr.bid.data(), edges, N, E, P, &op, &st, &items, &old_index_bytes);
    if (rc != g.code || g_code != g.code) differ(what, "code", rc, g.code);
    if (g_text != g.error) differ(what, "error text '" + g_text + "' / '" + g.error + "'");
    if (rc) return {rc, 0, 0, 0, 0, 0, 0, 0};
    const WsLayout L = ws_layout(ws_params(c, g, N, E, P));
    Plan np;
    ws_carve(&np, FAKE_ARENA, L);
    // scalars
    const struct { const char* n; long long a, b; } sc[] = {
        {"S", op.S, g.S}, {"max_n", op.max_n, g.max_n}, {"max_e", op.max_e, g.max_e}, {"is_fc", op.is_fc, g.is_fc}, {"fa_parts", op.fa_parts, g.fa_parts},
        {"n_tiles", op.n_tiles, (long long)g.tiles.size()}, {"n_tiles_big", op.n_tiles_big, (long long)g.tiles_big.size()},
        {"dual", op.dual, L.w.dual}, {"kvx_slots", op.kvx_slots, (long long)L.w.kvx_slots()},
        {"stn_ws_floats", (long long)op.stn_ws_floats, (long long)(L.bytes[WS_stn_ws] / sizeof(float))},
        {"total", (long long)op.ws_bytes, (long long)L.total}, {"index_bytes", (long long)old_index_bytes, (long long)L.index_bytes},
        {"bias_total", (long long)((const int64_t*)(old_stage.data() + (op.d_bias_ptr ? (char*)op.d_bias_ptr - FAKE_ARENA : 0)))[op.S - 1] +
                           (long long)c.H * (op.node_ptr[op.S] - op.node_ptr[op.S - 1]) * (op.node_ptr[op.S] - op.node_ptr[op.S - 1]), g.bias_total}};
    for (auto& s : sc) if (s.a != s.b) differ(what, s.n, s.a, s.b);
    if (memcmp(&op.flash_flops, &g.flash_flops, sizeof(double))) differ(what, "flash_flops", (long long)op.flash_flops, (long long)g.flash_flops);
    if (op.node_ptr != g.node_ptr) differ(what, "node_ptr");
    if (op.edge_ptr != g.edge_ptr) differ(what, "edge_ptr");
    // every buffer: exists in both or neither, same order, offset and size; the views
    size_t k = 0;
    int n_index = 0;
#define CHECK_BUF(m, T, rows, per, when, cols)                                                                                              \
    {                                                                                                                                         \
        const bool in_old = k < items.size() && items[k].dst == reinterpret_cast<void**>(&op.m);                                             \
        if (in_old != (L.bytes[WS_##m] != 0)) differ(what, #m " exists", in_old, L.bytes[WS_##m] != 0);                                       \
        if (in_old) {                                                                                                                         \
            if (items[k].bytes != L.bytes[WS_##m]) differ(what, #m " bytes", (long long)items[k].bytes, (long long)L.bytes[WS_##m]);           \
            if ((char*)op.m - FAKE_ARENA != (long long)L.off[WS_##m]) differ(what, #m " offset", (char*)op.m - FAKE_ARENA, (long long)L.off[WS_##m]); \
            if (L.off[WS_##m] & 255) differ(what, #m " alignment");                                                                           \
            n_index += WS_##m < WS_INDEX_END;                                                                                                 \
            ++k;                                                                                                                              \
        }                                                                                                                                     \
        if ((void*)op.m != (void*)np.m) differ(what, #m " pointer");                                                                           \
    }
    VLSAT_WS_BUFFERS(CHECK_BUF)
#undef CHECK_BUF
    if (k != items.size()) differ(what, "buffers the list does not have", (long long)items.size(), (long long)k);
    if (n_index != L.n_index) differ(what, "n_index", n_index, L.n_index);
    if (op.R1 != np.R1 || op.R2 != np.R2 || np.prob) differ(what, "R1 / R2");
    // the packed index tables, byte for byte (the padding is zero in both)
    std::vector<char> new_stage(L.index_bytes, 0);
    pack_index_tables(g, L, new_stage.data());
    if (L.index_bytes > old_stage.size()) differ(what, "staging size", (long long)old_stage.size(), (long long)L.index_bytes);
    if (memcmp(old_stage.data(), new_stage.data(), L.index_bytes))
        for (size_t i = 0; i < L.index_bytes; ++i)
            if (old_stage[i] != new_stage[i]) differ(what, "staging byte " + std::to_string(i), old_stage[i], new_stage[i]);
    if (real_arena) {
        // regions in order, disjoint, inside a buffer of exactly `total` bytes: every byte of every region written, then read back
        std::unique_ptr<char[]> arena(new char[L.total]);
        Plan rp;
        ws_carve(&rp, arena.get(), L);
        char* at = arena.get();
        int id = 0;
#define FILL_BUF(m, T, rows, per, when, cols)                                                                                 \
    if (L.bytes[WS_##m]) {                                                                                                      \
        if ((char*)rp.m < at) differ(what, #m " overlaps the buffer before it");                                               \
        memset(rp.m, id & 127, L.bytes[WS_##m]);                                                                              \
        at = (char*)rp.m + L.bytes[WS_##m];                                                                                     \
    } else if (rp.m) differ(what, #m " carved but absent");                                                                     \
    ++id;
        VLSAT_WS_BUFFERS(FILL_BUF)
#undef FILL_BUF
        if (at > arena.get() + L.total) differ(what, "end > total");
        id = 0;
#define READ_BUF(m, T, rows, per, when, cols)                                                                                 \
    if (L.bytes[WS_##m] && (*(char*)rp.m != (id & 127) || memcmp(rp.m, (char*)rp.m + 1, L.bytes[WS_##m] - 1))) differ(what, #m " overwritten by a later buffer"); \
    ++id;
        VLSAT_WS_BUFFERS(READ_BUF)
#undef READ_BUF
        if (rp.R1 != rp.Hbig || rp.R2 + (size_t)std::max<int64_t>(E, 1) * 512 != rp.Hbig + (size_t)std::max<int64_t>(E, 1) * 1024) differ(what, "R1 / R2 views");
    }
    return {0, L.total, L.w.dual, g.fa_parts, (int)g.tiles.size(), (int)g.tiles_big.size(), g.is_fc, g.S};
}

// the configurations of the enumeration on one graph: all 216, or (light) feature transform and layer count at two settings instead of six: 72;
// graphs of more than 8192 edges (where dual_stream 1 is 0) take 28 of those: every analysis switch, the layout switches not as a product
static void sweep(const Graph& g, bool light = true, int big_min = 4096) {
    for (int H : {4, 8, 16}) for (int scope : {0, 1}) for (int split : {0, 1}) for (int dual : {0, 1, 2}) for (int ft : {0, 1}) for (int layers : {1, 2, 3}) {
        if (light && !((ft == 0 && layers == 2) || (ft == 1 && layers == 3))) continue;
        if (g.E() > 8192 && !((dual == 2 && ft == 0) || (dual == 1 && ft == 1) || (dual == 0 && ft == 0 && H == 8))) continue;
        PlanCfg c;
        c.H = H; c.edge_scope = scope; c.fa_split = split; c.dual_stream = dual; c.feature_transform = ft; c.n_layers = layers; c.flash_bq_big_min = big_min;
        compare(g, c, ft ? 32 : 1 + (H + layers) % 3, g.E() <= 160 && H == 8 && layers == 2);
    }
}
static void expect(bool ok, const std::string& what, long long a = 0, long long b = 0) { if (!ok) differ(what, "expectation", a, b); }

static PlanCfg cfg(int H = 8, int scope = 0, int split = 1, int big_min = 4096) {
    PlanCfg c;
    c.H = H; c.edge_scope = scope; c.fa_split = split; c.flash_bq_big_min = big_min;
    return c;
}

static void time_plans();

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "time")) { time_plans(); return 0; }
    long at = 0;
    auto group = [&](const char* name, const std::string& more = "") { printf("%s -> ok %ld cases%s\n", name, g_cases - at, more.c_str()); at = g_cases; };

    // fully connected: one scene of 1, 2, 9, 12, 40, 200 nodes; 9 + 40 (the small scene uses fewer key parts than the plan); the bench batch; E = 0
    for (int n : {1, 2, 9, 12, 40, 200}) sweep(fc("fc " + std::to_string(n), {n}), n > 40);
    sweep(fc("fc 9+40", {9, 40}), false);
    {
        Outcome o = compare(fc("fc 9+40", {9, 40}), cfg(), 32);
        expect(o.fa_parts == 9 && o.n_tiles == 9 * 112 && o.is_fc == 1 && o.S == 2, "fc 9+40: (1 + 13) query tiles x 8 heads = 112 tiles, 9 parts", o.fa_parts, o.n_tiles);
    }
    sweep(repeat("bench batch 64 x 40", 64, 40));
    sweep(fc("fc 1+1+1, E = 0", {1, 1, 1}), false);
    { Graph g = repeat("5 nodes, E = 0", 1, 5, 0); sweep(g, false); expect(compare(g, cfg(), 4).is_fc == 0, "no edges among 5 nodes is not fully connected"); }
    { Graph g = repeat("3 x 4 nodes, E = 0", 3, 4, 0); sweep(g); }
    group("fully connected");

    // not fully connected
    {
        Graph g = fc("unsorted within a scene", {5, 7, 4});
        std::reverse(g.src.begin() + 20, g.src.begin() + 62); std::reverse(g.dst.begin() + 20, g.dst.begin() + 62);      // the second scene, backwards
        sweep(g, false);
        expect(compare(g, cfg(), 8).is_fc == 0, "unsorted: is_fc");
        Graph p; p.name = "pruned, one scene without edges";
        add_scene(p, 6, 11); add_scene(p, 5, 0); add_scene(p, 9, 40); add_scene(p, 3, 0);
        sweep(p, false);
        Graph m = fc("sorted, one edge missing", {6, 8});
        m.src.erase(m.src.begin() + 47); m.dst.erase(m.dst.begin() + 47);
        sweep(m, false);
        expect(compare(m, cfg(), 8).is_fc == 0, "one edge missing: is_fc");
        expect(compare(fc("fc 6+8", {6, 8}), cfg(), 8).is_fc == 1, "fc 6+8: is_fc");
    }
    group("not fully connected");

    // light tiles: 128 x 12 nodes is exactly 2048 tiles at 8 heads, one full and one light tile per scene and head; one scene fewer is below
    // the threshold; 128 scenes of 256 edges have no light tile; batches of mostly light tiles, with tile counts that are no multiple of 8 at 4 heads
    {
        Graph a = repeat("128 x 12 nodes", 128, 12), b = repeat("127 x 12 nodes", 127, 12);
        sweep(a); sweep(b);
        expect(compare(a, cfg(), 8).n_tiles == 2048 && compare(b, cfg(), 8).n_tiles == 2032, "128 / 127 x 12: tiles");
        sweep(repeat("128 x 17 nodes with 256 edges", 128, 17, 256));
        Graph c; c.name = "250 light scenes + 6 full";
        for (int s = 0; s < 256; ++s) (s % 43 == 7) ? add_scene(c, 17, 128) : add_scene(c, 6);
        sweep(c);
        Graph d; d.name = "509 light scenes + 4 full";
        for (int s = 0; s < 513; ++s) (s % 128 == 5) ? add_scene(d, 17, 128) : add_scene(d, 4);
        sweep(d);
        Graph e; e.name = "3 light scenes among 300 full";
        for (int s = 0; s < 303; ++s) (s % 101 == 50) ? add_scene(e, 6) : add_scene(e, 17, 256);
        sweep(e);
        Graph f; f.name = "261 scenes of 130 edges";
        for (int s = 0; s < 261; ++s) add_scene(f, 14, 130);
        sweep(f);
    }
    group("light tiles");

    // key split: 63 / 64 / 65 one-tile scenes are 504 / 512 / 520 tiles at 8 heads (2 parts | none | none), 252 at 4 heads (4 parts); one scene
    // alone wants more than 16 parts; scenes with 1, 2, 3 and 4 key tiles
    {
        for (int s : {31, 32, 33, 63, 64, 65, 127, 128}) sweep(repeat(std::to_string(s) + " x 6 nodes", s, 6));
        expect(compare(repeat("63 x 6", 63, 6), cfg(), 8).fa_parts == 2 && compare(repeat("64 x 6", 64, 6), cfg(), 8).fa_parts == 1 &&
                   compare(repeat("63 x 6", 63, 6), cfg(4), 8).fa_parts == 4 && compare(fc("fc 6", {6}), cfg(), 8).fa_parts == 16 &&
                   compare(repeat("63 x 6", 63, 6), cfg(8, 0, 0), 8).fa_parts == 1, "key split: parts");
        for (int n : {6, 8, 9, 11}) sweep(fc("fc " + std::to_string(n) + " (key tiles)", {n}));
        sweep(fc("fc 6+8+9+11", {6, 8, 9, 11}));
        sweep(fc("fc 40+3+26", {40, 3, 26}));
    }
    group("key split");

    // big tiles: eight scenes of 4096 edges are 1024 tiles of 256 queries at 8 heads; the smallest scene one edge below the minimum; sums of
    // 127 / 128 (8 heads), 255 / 256 (4 heads), 63 / 64 (16 heads) 256-query tiles per head; edge_scope 1 (in every sweep); another minimum
    {
        Graph a = repeat("8 x 4096 edges", 8, 70, 4096), b = a;
        b.name = "8 x 4096 edges, one of 4095"; b.src.pop_back(); b.dst.pop_back();
        sweep(a); sweep(b);
        expect(compare(a, cfg(), 8).n_tiles_big == 1024 && compare(b, cfg(), 8).n_tiles_big == 0 && compare(a, cfg(8, 1), 8).n_tiles_big == 0, "big tiles: 8 x 4096");
        for (int sum : {63, 64, 127, 128, 255, 256}) {
            Graph g; g.name = "256-query tiles per head: " + std::to_string(sum);
            const int k = sum / 17;                            // scenes of sum / k or one more tiles each: all of at least 4096 edges
            for (int i = 0; i < k; ++i) add_scene(g, 80, (int64_t)(sum / k + (i < sum % k)) * 256 - 3);
            sweep(g);
        }
        Graph s = repeat("40 x 1000 edges, minimum 1000 / 1001", 40, 40, 1000);
        sweep(s, true, 1000); sweep(s, true, 1001);
        expect(compare(s, cfg(8, 0, 1, 1000), 8).n_tiles_big == 40 * 8 * 4 && compare(s, cfg(8, 0, 1, 1001), 8).n_tiles_big == 0, "big tiles: minimum 1000");
    }
    group("big tiles");

    // refused graphs: code, text, and which of two faults is reported
    {
        const struct { const char* name; std::vector<int64_t> bid, src, dst; int code; const char* text; } bad[] = {
            {"batch id re-appears", {0, 0, 1, 0}, {0}, {1}, VLSAT_EINVAL, "batch_ids: nodes of a scene must be contiguous"},
            {"endpoint -1", {0, 0, 0}, {0, -1}, {1, 2}, VLSAT_EINVAL, "edge index out of range"},
            {"endpoint N", {0, 0, 0}, {0, 1}, {1, 3}, VLSAT_EINVAL, "edge index out of range"},
            {"edge across scenes", {0, 0, 1, 1}, {0, 1}, {1, 2}, VLSAT_EINVAL, "edge joins nodes of different scenes"},
            {"edges not grouped by scene", {0, 0, 1, 1}, {2, 0}, {3, 1}, VLSAT_EGRAPH, "edges are not grouped by scene in node order"},
            {"re-appearing id and a bad edge", {3, 3, 4, 3}, {0, 9}, {1, 0}, VLSAT_EINVAL, "batch_ids: nodes of a scene must be contiguous"},
            {"across scenes, then out of range", {0, 0, 1, 1}, {0, 1, 7}, {1, 2, 0}, VLSAT_EINVAL, "edge joins nodes of different scenes"},
            {"out of range, then ungrouped", {0, 0, 1, 1}, {2, 4, 0}, {3, 0, 1}, VLSAT_EINVAL, "edge index out of range"},
            {"ungrouped, then across scenes", {0, 0, 1, 1}, {2, 0, 1}, {3, 1, 2}, VLSAT_EGRAPH, "edges are not grouped by scene in node order"}};
        for (auto& b : bad) {
            Graph g; g.name = b.name; g.bid = b.bid; g.src = b.src; g.dst = b.dst;
            for (int scope : {0, 1}) {
                g_text.clear();
                expect(compare(g, cfg(8, scope), 8).code == b.code && g_text == b.text, std::string("refused: ") + b.name);
            }
        }
    }
    group("refused graphs");

    // the two-stream budget: one scene of 64 nodes, dual_stream 2; the edge count at which the second scratch set passes DUAL_WS_BUDGET, found
    // with the layout function on the counts alone, then old and new on the graph just under and just over (nothing of that size is allocated)
    {
        auto params = [](size_t E) {
            PlanGraph g; g.S = 1; g.bias_total = 8 * 64 * 64; g.tiles.resize(8 * ((E + 127) / 128));
            PlanCfg c = cfg();
            WsParams w = ws_params(c, g, 64, (int64_t)E, 8);
            return w;
        };
        size_t lo = 1 << 20, hi = 1 << 22;                 // lo: two streams, hi: one
        expect(ws_layout(params(lo)).w.dual && !ws_layout(params(hi)).w.dual, "budget bracket");
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; (ws_layout(params(mid)).w.dual ? lo : hi) = mid; }
        for (size_t E : {lo, hi}) {
            Outcome o = compare(repeat("64 nodes, " + std::to_string(E) + " edges", 1, 64, (int64_t)E), cfg(), 8);
            expect(o.dual == (E == lo), "budget: two streams just under, one just over", o.dual, (long long)E);
        }
        char more[96];
        snprintf(more, sizeof more, ", two streams up to %zu edges of one 64-node scene", lo);
        group("budget", more);
    }

    // size classes from 1 byte to 64 GiB, on both sides of each class boundary; the pool pick on hand-made pools
    {
        long n = 0;
        std::vector<Arena> none;
        for (size_t cls = size_t(1) << 20; cls <= size_t(64) << 30; cls = arena_size_class(cls + 1))
            for (size_t total : {cls - 1, cls, cls + 1, cls + cls / 4}) {
                int best; size_t want;
                legacy_arena(none, total, &best, &want);
                if (want != arena_size_class(total) || best != arena_pool_pick(none, total)) differ("size class", std::to_string(total), (long long)want, (long long)arena_size_class(total));
                expect(want >= total && (total <= (1 << 20) || want < total + total / 2 + 2), "size class within 1.5 x", (long long)total, (long long)want);
                ++n;
            }
        { int best; size_t want; legacy_arena(none, 1, &best, &want); expect(want == 1 << 20 && arena_size_class(1) == 1 << 20 && arena_size_class(0) == 1 << 20, "1 byte"); ++n; }
        const size_t M = 1 << 20;
        const std::vector<std::vector<size_t>> pools = {{}, {M}, {8 * M, 2 * M, 4 * M}, {3 * M, 3 * M, 2 * M}, {1000 * M, 6 * M}, {68 * M + 1, 68 * M}, {M / 2, 5 * M, 300 * M}};
        const int expected[][4] = {{-1, -1, -1, -1}, {0, 0, -1, -1}, {1, 1, 2, -1}, {2, 2, 0, -1}, {1, 1, 1, 0}, {-1, 1, 1, -1}, {0, 1, 1, 2}};      // (by hand)
        const size_t totals[4] = {1, M, 2 * M + 1, 240 * M};
        for (size_t i = 0; i < pools.size(); ++i) {
            std::vector<Arena> pool;
            for (size_t b : pools[i]) pool.push_back({nullptr, b});
            for (int t = 0; t < 4; ++t) {
                int best; size_t want;
                legacy_arena(pool, totals[t], &best, &want);
                if (best != arena_pool_pick(pool, totals[t])) differ("pool pick", std::to_string(i), best, arena_pool_pick(pool, totals[t]));
                expect(best == expected[i][t], "pool pick " + std::to_string(i) + " / " + std::to_string(t), best, expected[i][t]);
                ++n;
            }
        }
        printf("size classes -> ok %ld cases\n", n);
    }

    // the cases of tests/plan_cases.py: default configuration, P = 32
    {
        const struct { const char* name; Graph g; } cases[] = {{"one scene of 9 nodes", fc("", {9})}, {"two scenes of 3 and 5 nodes", fc("", {3, 5})}, {"one node, E = 0", fc("", {1})}};
        for (auto& c : cases) {
            Graph g = c.g; g.name = c.name;
            Outcome o = compare(g, PlanCfg(), 32);
            expect(o.is_fc == 1, "plan_cases: fully connected");
            printf("ws | %s | %zu\n", c.name, o.total);
        }
    }
    return 0;
}

// host time of plan creation, old and new interleaved: the 40-node scene and the bench batch (64 x 40 nodes), default configuration
static void time_plans() {
    for (int big : {0, 1}) {
        const Graph gr = big ? repeat("bench batch 64 x 40", 64, 40) : fc("one scene of 40 nodes", {40});
        const std::vector<int64_t> ed = gr.edges();
        const int reps = big ? 200 : 3000;
        const PlanCfg c;
        Ctx h = ctx_of(c);
        std::vector<char> stage((size_t)64 << 20);
        std::vector<double> told, tnew;
        size_t sink = 0;
        for (int r = 0; r < reps; ++r) {
            auto t0 = std::chrono::steady_clock::now();
            {
                Plan op; op.arena = FAKE_ARENA;
                Staging st{stage.data()};
                std::vector<OldItem> items; size_t ib = 0;
                legacy_plan_create(&h, gr.bid.data(), ed.data(), gr.N(), gr.E(), 32, &op, &st, &items, &ib);
                sink += op.ws_bytes;
            }
            auto t1 = std::chrono::steady_clock::now();
            {
                PlanGraph g = plan_graph_analyse(gr.bid.data(), ed.data(), gr.N(), gr.E(), c);
                const WsLayout L = ws_layout(ws_params(c, g, gr.N(), gr.E(), 32));
                Plan np; ws_carve(&np, FAKE_ARENA, L);
                pack_index_tables(g, L, stage.data());
                np.node_ptr = std::move(g.node_ptr); np.edge_ptr = std::move(g.edge_ptr);
                sink += L.total;
            }
            auto t2 = std::chrono::steady_clock::now();
            told.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
            tnew.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
        }
        std::sort(told.begin(), told.end()); std::sort(tnew.begin(), tnew.end());
        auto q = [&](const std::vector<double>& v, double f) { return v[(size_t)(f * (v.size() - 1))]; };
        printf("time | %s | %d repetitions | old: median %.1f us (quartiles %.1f .. %.1f) | new: median %.1f us (quartiles %.1f .. %.1f) | %zu\n", gr.name.c_str(), reps,
               q(told, 0.5), q(told, 0.25), q(told, 0.75), q(tnew, 0.5), q(tnew, 0.25), q(tnew, 0.75), sink % 10);
    }
}
