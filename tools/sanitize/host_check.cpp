// host_check.cpp — AddressSanitizer / UBSan driver for the host C/C++ code
// (sanitizers run on the host restatement, never on the GPU).
//
// Built by tools/sanitize/Makefile from the SOURCES of librt_host (JSON
// parser, schema loader, IR, PNG writer), the device-table compiler
// (scene_compile.cpp), the frame planners (frame_plan.cpp) and the C oracle,
// all with -fsanitize=address,undefined; tests/test_sanitize.py runs it over
// the example, torture and deep scenes plus malformed JSON.  Per scene: load,
// compile the device object table, pick the frame's kernel variant, compile
// every node's own programs (the node queries') and pick their kernels, render
// a band of rows on the oracle in both modes, toByte, PNG; then the frame
// planners over the shapes of tests/test_frame_plan.py and the jitter cache's
// logic (jitter_cache.cpp) over the scripts of tests/test_jitter_cache.py.
// Exit 0 = no sanitizer report.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "frame_plan.hpp"
#include "jitter_cache.hpp"
#include "oracle.h"
#include "rt.h"
#include "scene_compile.hpp"

static int check_file(const char* path, const char* png_out) {
    rt_scene* s = nullptr;
    const int rc = rt_scene_load_json_file(path, &s);
    if (rc != RT_OK) {
        std::printf("load %s: rc=%d %s\n", path, rc, rt_last_error());
        return 0;   // an error path is a valid outcome (exercised for the sanitizers)
    }
    const rt_scene_desc* d = rt_scene_get_desc(s);
    rtamd::CompiledScene cs = rtamd::compile_scene(*d);
    for (int mode = 0; mode < 2; ++mode)
        for (int flags : {0, (int)RT_FLAG_COUNT_OPS, (int)RT_FLAG_NO_CULL, (int)RT_FLAG_NO_BVH, (int)RT_FLAG_FP32}) {
            rtamd::KernelVariant v;
            (void)rtamd::pick_variant(cs, *d, mode, flags, true, &v);   // (a refusal is a valid outcome)
            if (mode == 0) (void)rtamd::pick_query_variant(cs, *d, flags, &v);   // (the ray queries' kernel choice)
            if (mode == 0) (void)rtamd::pick_radiance_variant(cs, *d, flags, &v);   // (the radiance queries')
            if (mode == 0) (void)rtamd::pick_shade_variant(cs, *d, flags, &v);   // (the shading queries')
        }
    // every node's own programs and their kernel choice (the node queries': compile_node_program, pick_node_variant)
    size_t node_ops = 0;
    for (int node = 0; node < d->n_nodes; ++node)
        for (int kind : {(int)rtamd::kNodeIsect, (int)rtamd::kNodeIvl}) {
            const rtamd::NodeProgram p = rtamd::compile_node_program(*d, node, kind);
            rtamd::KernelVariant v;
            (void)rtamd::pick_node_variant(*d, node, p, 0, &v);   // (a refusal is a valid outcome)
            node_ops += p.ops.size();
        }
    int W = rt_camera_width(&d->camera), H = rt_camera_height(&d->camera);
    if (W > 64) W = 64;
    if (H > 48) H = 48;
    std::vector<double> fb((size_t)W * H * 3);
    for (int mode = 0; mode < 2; ++mode) {
        oracle_stats st{};
        if (oracle_render_rows(d, W, H, mode, 0, H, fb.data(), &st, 2) != 0) {
            std::printf("oracle failed on %s\n", path);
            rt_scene_destroy(s);
            return 1;
        }
        std::vector<uint8_t> rgb((size_t)W * H * 3);
        rt_framebuffer_to_rgb8(fb.data(), (size_t)W * H, rgb.data());
        if (rt_write_png(png_out, rgb.data(), W, H, 3) != RT_OK) {
            std::printf("png failed\n");
            rt_scene_destroy(s);
            return 1;
        }
    }
    std::printf("ok %s %dx%d objs=%zu ops=%zu fold=%zu node_ops=%zu\n", path, W, H, cs.objs.size(), cs.ops.size(),
                cs.fold.size(), node_ops);
    rt_scene_destroy(s);
    return 0;
}

// The frame planners at the shapes tests/test_frame_plan.py asserts on (here
// only for the sanitizers' sake: every index they compute is exercised).
static size_t check_plans() {
    size_t sum = 0;
    const int dist[][4] = {{2160, 8, 0, 4}, {4320, 8, 1, 2}, {2160, 3, 0, 4}, {4320, 3, 1, 2}, {17, 4, 0, 4},
                           {17, 4, 1, 2},   {5, 8, 0, 4},    {5, 8, 1, 2},    {1, 1, 0, 4},    {1, 1, 1, 2}};
    for (const auto& c : dist)
        for (int kind = 0; kind < 2; ++kind)
            for (int rank = 0; rank < c[1]; ++rank) {
                const rtamd::DistPlan p = rtamd::plan_dist_frame(c[0], c[1], rank, c[2], kind ? 0 : rtamd::root_shed(c[2]),
                                                                 c[3], rank == 0);
                sum += p.rows.size() + p.bounds.size() + p.rowtab.size();
            }
    const std::vector<std::vector<int32_t>> std_rows = {{4, 3, 2, 1, 0}, {0, 2, 4}, {2, 0, 1}};
    for (const auto& rows : std_rows) sum += rtamd::plan_std_frame(3, 5, rows.data(), (int)rows.size(), 64 * 624).jranges.size();
    struct PaperCase {
        int W, H;
        std::vector<int32_t> rows;
        std::vector<std::pair<int, int>> calls;
    };
    auto iota = [](int a, int b) {
        std::vector<int32_t> v;
        for (int i = a; i < b; ++i) v.push_back(i);
        return v;
    };
    std::vector<int32_t> split = iota(0, 30), tail = iota(60, 70);
    split.insert(split.end(), tail.begin(), tail.end());
    const std::vector<PaperCase> paper = {{17, 1, iota(0, 1), {{0, 1}}},       {17, 2, iota(0, 2), {{0, 2}}},
                                          {17, 31, iota(0, 31), {{0, 30}, {30, 31}}}, {1, 70, split, {{0, 40}}},
                                          {5, 70, iota(0, 60), {{0, 30}, {30, 60}}}};
    for (const PaperCase& pc : paper) {
        const rtamd::PaperPlan p = rtamd::plan_paper_frame(7, pc.W, pc.H, RT_MODE_PAPER, 0, pc.rows.data(), (int)pc.rows.size());
        rtamd::PaperCalls calls;
        calls.reset(&p);
        std::vector<uint32_t> gc;
        for (size_t k = 0; k < pc.calls.size(); ++k) {
            const rtamd::PaperCalls::Call c = calls.next_call(pc.calls[k].first, pc.calls[k].second, k + 1);
            sum += c.list->size() + c.wait.size();
        }
        gc.assign((size_t)calls.list_used() / 8, 3);
        std::vector<uint32_t> cost;
        calls.group_costs(gc.data(), cost);
        calls.rollback();
        // the same frame again, costliest blocks first
        calls.reset(&p);
        for (size_t k = 0; k < pc.calls.size(); ++k) sum += calls.next_call(pc.calls[k].first, pc.calls[k].second, 1, &cost).list->size();
        sum += p.aux_ints() + p.gtime_words() + (size_t)p.logical_isect;
    }
    return sum;
}

// The jitter cache's logic over host memory (jitter_cache.hpp
// jitter_cache_sim), at the scripts of tests/test_jitter_cache.py: hits,
// same-size keys, an abandoned frame, evictions, the uncached buffer and
// allocation failures, so that every buffer the cache hands out, frees or
// keeps is exercised under the sanitizers.  Returns the number of scripts
// that reported a stale buffer, a leak or a double free.
static int check_jitter_cache() {
    const int64_t e3 = (int64_t)rtamd::JitterCache::entry_bytes(3 * 16 * 2 * sizeof(double), 6);
    const int64_t big = 1 << 20;
    struct Script {
        int64_t budget;
        std::vector<std::vector<int64_t>> ops;   // {op, W, row0, n_rows, arg}
    };
    const std::vector<int64_t> A = {0, 2, 0, 3, 0}, B = {0, 2, 3, 3, 0}, C = {0, 2, 6, 3, 0}, A_left = {1, 2, 0, 3, 0},
                               wide = {0, 3, 0, 2, 0}, tall = {0, 2, 0, 4, 0}, small = {0, 2, 0, 2, 0};
    const auto fail = [](int64_t n) { return std::vector<int64_t>{3, 0, 0, 0, n}; };
    const std::vector<Script> scripts = {
        {big, {A, A, wide, B, A, wide, B, {0, 2, 0, 3, 56}, A}},   // (arg of a frame: its height, part of the key)
        {big, {A_left, A, A, A_left, A}},
        {2 * e3, {A, B, A, C, A, B}},
        {e3, {A, small, A, small, small, tall, A}},
        {0, {A, A, B, A}},
        {e3 - 1, {A, A, B, A, {5, 0, 0, 0, 0}, A}},
        {big, {A, B, {4, 0, 0, 0, e3}, A, C, C, {2, 0, 0, 0, 0}, A}},
        {big, {A, fail(1), B, B, A}},
        {e3, {A, fail(1), tall}},
        {big, {A, fail(3), B, B}},
    };
    int bad = 0;
    for (const Script& s : scripts) {
        std::vector<int64_t> ops, out(8 * (s.ops.size() + 1));
        for (const auto& o : s.ops) ops.insert(ops.end(), o.begin(), o.end());
        const int64_t release[5] = {5, 0, 0, 0, 0};
        ops.insert(ops.end(), release, release + 5);
        bad += rtamd::jitter_cache_sim(ops.data(), (int)s.ops.size() + 1, s.budget, out.data()) != 0;
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: host_check <out.png> <scene.json>...\n");
        return 2;
    }
    int bad = 0;
    for (int i = 2; i < argc; ++i) bad += check_file(argv[i], argv[1]);
    // malformed inputs through the text entry point (error paths)
    const char* broken[] = {"", "{", "{\"objects\": [{\"sphere\": {}}]}", "[1, 2", "{\"screen\": {\"dpi\": \"x\"}}",
                            "{\"objects\": [{\"csg\": {\"operator\": \"xor\"}}]}", "\xef\xbb\xbf{}", "nul\0l"};
    for (const char* t : broken) {
        rt_scene* s = nullptr;
        if (rt_scene_load_json_text(t, std::strlen(t), &s) == RT_OK) rt_scene_destroy(s);
    }
    std::printf("plans %zu\n", check_plans());
    const int bad_cache = check_jitter_cache();
    std::printf("jitter cache: %d bad scripts\n", bad_cache);
    return bad || bad_cache ? 1 : 0;
}
