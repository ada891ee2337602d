// Host-only program of tests/gate_host.py: it includes the library's internal header, never opens a device and prints
//   select   one line per input of gate_select: "H A terms gate_bf16 heads_mfma heads_bf16 -> kernel fuse_agg twin row_map0"
//   refuse   what launch_gate answers to an `agg`, a twin or a row_map = 0 handed to a kernel that does not implement it:
//            "kernel extra -> return code | message".  The pointers are never dereferenced: a refusal comes before any launch.
#include <cstdio>
#include <cstring>

#include "kernels.h"
#include "vlsat.h"

using namespace vlsat;

static const char* NAMES[] = {"valu", "f32", "f32_heads", "16", "16_heads"};

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "select")) {
        for (int H : {4, 8, 16})
            for (int A : {128, 256, 512})
                for (int terms : {0, 1, 3})
                    for (int bf16 = 0; bf16 < 2; ++bf16)
                        for (int hm = 0; hm < 3; ++hm)
                            for (int hb = 0; hb < 2; ++hb) {
                                const GateChoice c = gate_select(H, 512 / H, A / H, terms, bf16, hm, hb);
                                printf("%d %d %d %d %d %d -> %s %d %d %d\n", H, A, terms, bf16, hm, hb, NAMES[c.kernel], c.fuse_agg, c.twin, c.row_map0);
                            }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "refuse")) {
        static float buf[4];
        static int32_t idx[4];
        struct Geo { GateKernel k; int H, dk, dox, terms; } geos[] = {{GATE_VALU, 16, 32, 8, 0}, {GATE_VALU, 8, 64, 32, 0}, {GATE_F32_HEADS, 16, 32, 8, 0},
                                                                  {GATE_F32_HEADS, 4, 128, 128, 0}, {GATE_16_HEADS, 16, 32, 8, 3}, {GATE_16_HEADS, 8, 64, 32, 1}};
        for (const Geo& g : geos)
            for (int extra = 0; extra < 3; ++extra) {
                GateArgs a{};
                a.kproj = a.node = a.w0k = a.w3 = a.b3 = buf; a.gated = buf; a.src = a.dst = idx;
                a.ld_node = 1024; a.gq_off = 0; a.v_off = 512; a.n_edges = 1;
                GateArgs b = a;
                if (extra == 0) { a.agg = buf; a.ld_agg = 768; }
                if (extra == 2) a.row_map = 0;
                const int r = launch_gate(g.k, a, g.H, g.dk, g.dox, g.terms, 0, nullptr, extra == 1 ? &b : nullptr);
                printf("%s %s -> %d | %s\n", NAMES[g.k], extra == 0 ? "agg" : extra == 1 ? "twin" : "row_map0", r, r ? vlsat_last_error() : "");
            }
        return 0;
    }
    return 2;
}
