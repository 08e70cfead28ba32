// registration_host_check.hip: the host side of both registration rules (csrc/rwh_bundle.hip, csrc/rwh_camera.hip through
// csrc/rwh_edge_blocks.h) driven from a main of its own, for a run under the host sanitizers.  No GPU is used: of the two device
// entry points only the refusals are called, which return before any launch.  Every output is a heap block of exactly the size the
// ABI states, so a write past one is seen.  Build and run from the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Iinclude -Iransac_with_homography_amd/csrc -ffp-contract=off \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined tools/registration_host_check.hip \
//         ransac_with_homography_amd/csrc/rwh_bundle.hip ransac_with_homography_amd/csrc/rwh_camera.hip -o /tmp/registration_host_check
//   /tmp/registration_host_check
// It covers: the 13 edge sizes 0 .. 600 in one call with mask rows of 10, 9 and 1 words, twin against twin on the rows a shorter
// mask row leaves; the steps at three anchors, at lambda 0 and 1e-3, both focal models; an image no edge touches (SINGULAR, delta
// zero); n = 1; every refusal of the six entry points.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rwh.h"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            printf("FAILED line %d: %s\n", __LINE__, #c);                \
            return 1;                                                    \
        }                                                                \
    } while (0)

static uint64_t state = 88172645463325252ull;
static double uniform() {       // xorshift64 -> [0, 1)
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
}

int main() {
    const int sizes[13] = {0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257, 600};
    const int E = 13, n = 5;
    std::vector<int32_t> offsets(E + 1, 0), edges;
    for (int e = 0; e < E; ++e) offsets[e + 1] = offsets[e] + sizes[e];
    for (int d = 0; d < n; ++d)
        for (int s = d + 1; s < n; ++s) { edges.push_back(s); edges.push_back(d); }
    for (int e = 10; e < E; ++e) { edges.push_back(edges[2 * (e - 10) + 1]); edges.push_back(edges[2 * (e - 10)]); }
    const int total = offsets[E];
    std::vector<float> pa(2 * total), pb(2 * total);
    std::vector<double> T(9 * E), rec(15 * E);
    for (int e = 0; e < E; ++e) {
        const double shift = 30.0 * (edges[2 * e] - edges[2 * e + 1]), yaw = 0.12 * (edges[2 * e] - edges[2 * e + 1]);
        const double t[9] = {1.01, 0.02, shift, -0.01, 0.99, 3.0, 1e-4, -1e-4, 1.0};
        for (int i = 0; i < 9; ++i) T[9 * e + i] = t[i] / fabs(shift);
        const double r[15] = {cos(yaw), 0.0, sin(yaw), 0.0, 1.0, 0.0, -sin(yaw), 0.0, cos(yaw), 150.0, 79.5, 59.5, 152.0, 79.5, 59.5};
        for (int i = 0; i < 15; ++i) rec[15 * e + i] = r[i];
        for (int i = offsets[e]; i < offsets[e + 1]; ++i) {
            pa[2 * i] = (float)(160.0 * uniform());
            pa[2 * i + 1] = (float)(120.0 * uniform());
            pb[2 * i] = (float)(pa[2 * i] + shift + uniform());
            pb[2 * i + 1] = (float)(pa[2 * i + 1] + uniform());
        }
    }
    const int widths[3] = {10, 9, 1};
    std::vector<double> bblocks[3], cblocks[3];
    for (int v = 0; v < 3; ++v) {
        const int words = widths[v];
        std::vector<uint64_t> masks((size_t)E * words);
        for (size_t i = 0; i < masks.size(); ++i) masks[i] = v == 0 ? ~0ull : 0xF7FFFFFFFFFFFFEFull;
        std::vector<int32_t> count(E), status(E);
        bblocks[v].assign((size_t)E * RWH_BUNDLE_BLOCK, -1.0);
        CHECK(rwh_host_bundle_blocks(pa.data(), pb.data(), offsets.data(), E, masks.data(), words, T.data(), bblocks[v].data(), count.data(),
                                     status.data()) == RWH_OK);
        for (int e = 0; e < E; ++e) CHECK(status[e] == RWH_BUNDLE_OK && count[e] <= sizes[e] && count[e] <= 64 * words && (sizes[e] == 0) == (count[e] == 0));
        for (double x : bblocks[v]) CHECK(isfinite(x));
        cblocks[v].assign((size_t)E * RWH_CAMERA_BLOCK, -1.0);
        CHECK(rwh_host_camera_blocks(pa.data(), pb.data(), offsets.data(), E, masks.data(), words, rec.data(), cblocks[v].data(), count.data(),
                                     status.data()) == RWH_OK);
        for (int e = 0; e < E; ++e) CHECK(status[e] == RWH_BUNDLE_OK && count[e] <= sizes[e] && count[e] <= 64 * words);
        for (double x : cblocks[v]) CHECK(isfinite(x));
    }
    // an edge that fits into the shorter mask row has the same bits under both widths of the same words
    CHECK(memcmp(bblocks[1].data(), bblocks[2].data(), sizeof(double) * 5 * RWH_BUNDLE_BLOCK) == 0);
    CHECK(memcmp(cblocks[1].data(), cblocks[2].data(), sizeof(double) * 5 * RWH_CAMERA_BLOCK) == 0);

    int32_t st = -1;
    const int anchors[3] = {0, 2, 4};
    const double lambdas[2] = {0.0, 1e-3};
    for (int anchor : anchors)
        for (double lambda : lambdas) {
            std::vector<double> delta(8 * n, -1.0);
            CHECK(rwh_host_bundle_step(n, anchor, edges.data(), E, bblocks[0].data(), lambda, delta.data(), &st) == RWH_OK && st == RWH_BUNDLE_OK);
            for (int i = 0; i < 8 * n; ++i) CHECK(isfinite(delta[i]) && ((i / 8 == anchor) == (delta[i] == 0.0)));
            for (int focals : {RWH_CAMERA_FOCAL_SHARED, RWH_CAMERA_FOCAL_PER_IMAGE}) {
                std::vector<double> cdelta(4 * n, -1.0);
                CHECK(rwh_host_camera_step(n, anchor, focals, edges.data(), E, cblocks[0].data(), lambda, cdelta.data(), &st) == RWH_OK);
                CHECK(st == RWH_BUNDLE_OK);
                for (int i = 0; i < 4 * n; ++i) CHECK(isfinite(cdelta[i]) && (i / 4 != anchor || i % 4 == 3 || cdelta[i] == 0.0));
                if (focals == RWH_CAMERA_FOCAL_SHARED)
                    for (int i = 1; i < n; ++i) CHECK(cdelta[4 * i + 3] == cdelta[3]);
            }
        }
    {   // image 5 of six: no edge touches it
        std::vector<double> delta(8 * 6, -1.0), cdelta(4 * 6, -1.0);
        CHECK(rwh_host_bundle_step(6, 0, edges.data(), E, bblocks[0].data(), 1e-3, delta.data(), &st) == RWH_OK && st == RWH_BUNDLE_SINGULAR);
        for (double x : delta) CHECK(x == 0.0);
        CHECK(rwh_host_camera_step(6, 0, RWH_CAMERA_FOCAL_PER_IMAGE, edges.data(), E, cblocks[0].data(), 1e-3, cdelta.data(), &st) == RWH_OK);
        CHECK(st == RWH_BUNDLE_SINGULAR);
        for (double x : cdelta) CHECK(x == 0.0);
        CHECK(rwh_host_camera_step(6, 0, RWH_CAMERA_FOCAL_SHARED, edges.data(), E, cblocks[0].data(), 1e-3, cdelta.data(), &st) == RWH_OK);
        CHECK(st == RWH_BUNDLE_SINGULAR);
    }
    {   // n = 1 has no pair of two different images: every edge list is refused
        std::vector<double> delta(8, -1.0);
        const int32_t self[2] = {0, 0}, out[2] = {1, 0};
        CHECK(rwh_host_bundle_step(1, 0, self, 1, bblocks[0].data(), 1e-3, delta.data(), &st) == RWH_E_INVALID);
        CHECK(rwh_host_bundle_step(1, 0, out, 1, bblocks[0].data(), 1e-3, delta.data(), &st) == RWH_E_INVALID);
        CHECK(rwh_host_camera_step(1, 0, RWH_CAMERA_FOCAL_SHARED, self, 1, cblocks[0].data(), 1e-3, delta.data(), &st) == RWH_E_INVALID);
    }
    // the refusals
    std::vector<uint64_t> ones((size_t)E * 10, ~0ull);
    std::vector<int32_t> count(E), status(E);
    std::vector<double> delta(8 * n);
    typedef int (*blocks_fn)(const float*, const float*, const int32_t*, int, const uint64_t*, int, const double*, double*, int32_t*, int32_t*);
    const blocks_fn twins[2] = {rwh_host_bundle_blocks, rwh_host_camera_blocks};
    const double* records[2] = {T.data(), rec.data()};
    for (int r = 0; r < 2; ++r) {
        double* blocks = r == 0 ? bblocks[0].data() : cblocks[0].data();
        CHECK(twins[r](nullptr, pb.data(), offsets.data(), E, ones.data(), 10, records[r], blocks, count.data(), status.data()) == RWH_E_INVALID);
        CHECK(twins[r](pa.data(), nullptr, offsets.data(), E, ones.data(), 10, records[r], blocks, count.data(), status.data()) == RWH_E_INVALID);
        CHECK(twins[r](pa.data(), pb.data(), nullptr, E, ones.data(), 10, records[r], blocks, count.data(), status.data()) == RWH_E_INVALID);
        CHECK(twins[r](pa.data(), pb.data(), offsets.data(), E, nullptr, 10, records[r], blocks, count.data(), status.data()) == RWH_E_INVALID);
        CHECK(twins[r](pa.data(), pb.data(), offsets.data(), E, ones.data(), 10, nullptr, blocks, count.data(), status.data()) == RWH_E_INVALID);
        CHECK(twins[r](pa.data(), pb.data(), offsets.data(), E, ones.data(), 10, records[r], nullptr, count.data(), status.data()) == RWH_E_INVALID);
        CHECK(twins[r](pa.data(), pb.data(), offsets.data(), E, ones.data(), 10, records[r], blocks, nullptr, status.data()) == RWH_E_INVALID);
        CHECK(twins[r](pa.data(), pb.data(), offsets.data(), E, ones.data(), 10, records[r], blocks, count.data(), nullptr) == RWH_E_INVALID);
        for (int n_edges : {0, -1, RWH_BUNDLE_MAX_EDGES + 1})
            CHECK(twins[r](pa.data(), pb.data(), offsets.data(), n_edges, ones.data(), 10, records[r], blocks, count.data(), status.data()) == RWH_E_INVALID);
        CHECK(twins[r](pa.data(), pb.data(), offsets.data(), E, ones.data(), 0, records[r], blocks, count.data(), status.data()) == RWH_E_INVALID);
    }
    // the device entry points: only what they refuse before a launch
    CHECK(rwh_bundle_blocks(nullptr, pb.data(), offsets.data(), E, ones.data(), 10, T.data(), bblocks[0].data(), count.data(), status.data(), nullptr) == RWH_E_INVALID);
    CHECK(rwh_bundle_blocks(pa.data(), pb.data(), offsets.data(), 0, ones.data(), 10, T.data(), bblocks[0].data(), count.data(), status.data(), nullptr) == RWH_E_INVALID);
    CHECK(rwh_bundle_blocks(pa.data(), pb.data(), offsets.data(), RWH_BUNDLE_MAX_EDGES + 1, ones.data(), 10, T.data(), bblocks[0].data(), count.data(), status.data(), nullptr) == RWH_E_INVALID);
    CHECK(rwh_bundle_blocks(pa.data(), pb.data(), offsets.data(), E, ones.data(), 0, T.data(), bblocks[0].data(), count.data(), status.data(), nullptr) == RWH_E_INVALID);
    CHECK(rwh_camera_blocks(pa.data(), pb.data(), offsets.data(), E, ones.data(), 10, nullptr, cblocks[0].data(), count.data(), status.data(), nullptr) == RWH_E_INVALID);
    CHECK(rwh_camera_blocks(pa.data(), pb.data(), offsets.data(), 0, ones.data(), 10, rec.data(), cblocks[0].data(), count.data(), status.data(), nullptr) == RWH_E_INVALID);
    CHECK(rwh_camera_blocks(pa.data(), pb.data(), offsets.data(), RWH_BUNDLE_MAX_EDGES + 1, ones.data(), 10, rec.data(), cblocks[0].data(), count.data(), status.data(), nullptr) == RWH_E_INVALID);
    CHECK(rwh_camera_blocks(pa.data(), pb.data(), offsets.data(), E, ones.data(), 0, rec.data(), cblocks[0].data(), count.data(), status.data(), nullptr) == RWH_E_INVALID);
    // the steps
    const double* bb = bblocks[0].data();
    const double* cb = cblocks[0].data();
    const int32_t bad_edges[3][2] = {{1, 5}, {-1, 2}, {2, 2}};
    const double nan = NAN, inf = INFINITY;
    CHECK(rwh_host_bundle_step(n, 0, nullptr, E, bb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
    CHECK(rwh_host_bundle_step(n, 0, edges.data(), E, nullptr, 1e-3, delta.data(), &st) == RWH_E_INVALID);
    CHECK(rwh_host_bundle_step(n, 0, edges.data(), E, bb, 1e-3, nullptr, &st) == RWH_E_INVALID);
    CHECK(rwh_host_bundle_step(n, 0, edges.data(), E, bb, 1e-3, delta.data(), nullptr) == RWH_E_INVALID);
    CHECK(rwh_host_camera_step(n, 0, 0, nullptr, E, cb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
    CHECK(rwh_host_camera_step(n, 0, 0, edges.data(), E, nullptr, 1e-3, delta.data(), &st) == RWH_E_INVALID);
    CHECK(rwh_host_camera_step(n, 0, 0, edges.data(), E, cb, 1e-3, nullptr, &st) == RWH_E_INVALID);
    CHECK(rwh_host_camera_step(n, 0, 0, edges.data(), E, cb, 1e-3, delta.data(), nullptr) == RWH_E_INVALID);
    for (int images : {0, -3, RWH_SEQ_MAX_IMAGES + 1}) {
        CHECK(rwh_host_bundle_step(images, 0, edges.data(), E, bb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
        CHECK(rwh_host_camera_step(images, 0, 0, edges.data(), E, cb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
    }
    for (int anchor : {-1, n}) {
        CHECK(rwh_host_bundle_step(n, anchor, edges.data(), E, bb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
        CHECK(rwh_host_camera_step(n, anchor, 0, edges.data(), E, cb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
    }
    for (int n_edges : {0, -1, RWH_BUNDLE_MAX_EDGES + 1}) {
        CHECK(rwh_host_bundle_step(n, 0, edges.data(), n_edges, bb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
        CHECK(rwh_host_camera_step(n, 0, 0, edges.data(), n_edges, cb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
    }
    for (double lambda : {-1.0, nan, inf}) {
        CHECK(rwh_host_bundle_step(n, 0, edges.data(), E, bb, lambda, delta.data(), &st) == RWH_E_INVALID);
        CHECK(rwh_host_camera_step(n, 0, 0, edges.data(), E, cb, lambda, delta.data(), &st) == RWH_E_INVALID);
    }
    for (const auto& edge : bad_edges) {
        CHECK(rwh_host_bundle_step(n, 0, edge, 1, bb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
        CHECK(rwh_host_camera_step(n, 0, 0, edge, 1, cb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
    }
    for (int focals : {-1, 2}) CHECK(rwh_host_camera_step(n, 0, focals, edges.data(), E, cb, 1e-3, delta.data(), &st) == RWH_E_INVALID);
    printf("registration host check: ok\n");
    return 0;
}
