// host_build_check.cpp -- khp_host_build on the scenes of tools/dump_build_cases.py,
// a stand-alone program for sanitizer builds of the host builder (make asan-check:
// scene.cpp and this file with -fsanitize=address,undefined; nothing is preloaded).
// Each case states the status it expects; a built tree is checked for the basics
// (ids a permutation, leaf ranges tiling [0, n)), everything else is the sanitizers'.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kirk_hip.h"

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    setvbuf(stdout, nullptr, _IOLBF, 0);  // a sanitizer abort must not swallow the lines before it
    int n_cases = 0, n_bad = 0;
    for (;;) {
        uint32_t len = 0, head[3];
        if (fread(&len, 4, 1, f) != 1) break;
        std::string name(len, ' ');
        if (fread(&name[0], 1, len, f) != len || fread(head, 4, 3, f) != 3) return 2;
        const uint32_t want = head[0], nt = head[1], nc = head[2], n = nt + nc;
        std::vector<float> tv, tn, cb, ca;
        std::vector<uint32_t> tm, cm;
        if (!rd(f, tv, 9 * (size_t)nt) || !rd(f, tn, 9 * (size_t)nt) || !rd(f, tm, nt) || !rd(f, cb, 4 * (size_t)nc) ||
            !rd(f, ca, 4 * (size_t)nc) || !rd(f, cm, nc))
            return 2;
        khp_material mat;
        memset(&mat, 0, sizeof(mat));
        khp_scene s;
        memset(&s, 0, sizeof(s));
        s.n_tris = nt;
        s.tri_v = tv.data();
        s.tri_n = tn.data();
        s.tri_mat = tm.data();
        s.n_cones = nc;
        s.cone_base_r0 = cb.data();
        s.cone_apex_r1 = ca.data();
        s.cone_mat = cm.data();
        s.n_materials = 1;
        s.materials = &mat;
        uint32_t nn = 0, depth = 0;
        khp_status st = khp_host_build(&s, &nn, &depth, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        bool ok = (uint32_t)st == want;
        if (ok && st == KHP_OK) {
            std::vector<float> boxes(6 * (size_t)nn), bounds(9 * (size_t)n), rec(16 * (size_t)n);
            std::vector<int32_t> first(nn), count(nn), ids(n);
            st = khp_host_build(&s, &nn, &depth, boxes.data(), first.data(), count.data(), ids.data(), bounds.data(),
                                rec.data());
            ok = st == KHP_OK;
            std::vector<char> seen(n, 0);
            for (uint32_t i = 0; ok && i < n; ++i) {
                ok = ids[i] >= 0 && (uint32_t)ids[i] < n && !seen[ids[i]];
                if (ok) seen[ids[i]] = 1;
            }
            int64_t next = 0;
            for (uint32_t i = 0; ok && i < nn; ++i)
                if (count[i] > 0) {
                    ok = first[i] == next;
                    next += count[i];
                }
            ok = ok && next == (int64_t)n;
        }
        printf("%-44s %8u objects  status %d (expected %u)  %u nodes  depth %u  %s\n", name.c_str(), n, (int)st, want,
               nn, depth, ok ? "ok" : "FAILED");
        ++n_cases;
        n_bad += !ok;
    }
    fclose(f);
    printf("%d cases, %d failed\n", n_cases, n_bad);
    return n_bad ? 1 : 0;
}
