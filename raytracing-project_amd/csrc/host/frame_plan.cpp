// frame_plan.cpp — see frame_plan.hpp.  Host-only: no HIP include.
#include "frame_plan.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>

#include "rt_internal.hpp"

namespace rtamd {

namespace {
int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e && *e ? std::atoi(e) : dflt;
}
bool env_on(const char* name) {   // (NAME=0: measurement A/B)
    const char* e = std::getenv(name);
    return !(e && *e == '0');
}

// every object a sphere, half-space or pokeball (no transform or CSG object:
// the plain kernels, rt_device.hpp CntPlain)
bool plain_scene(const CompiledScene& cs) {
    for (const auto& o : cs.objs)
        if (o.kind != OBJ_SPHERE && o.kind != OBJ_HALF && o.kind != OBJ_POKE && o.kind != OBJ_NEVER &&
            o.kind != OBJ_GROUP)
            return false;
    return true;
}

// Stack tiers: the common kernels, else the big-stack build (rtdb, *big), else
// refuse.  frames: the reflection / refraction frames the trace needs.
int stack_tier(int max_ray_depth, int max_ivl_depth, const rt_scene_desc& d, int frames, bool fp32, bool* big) {
    *big = false;
    if (max_ray_depth > kMaxRayStack || max_ivl_depth > kMaxIvlSpill + 2 || frames > kMaxDepth) {
        if (max_ray_depth > kBigRayStack || max_ivl_depth > kBigIvlSpill + 2 || frames > kBigDepth) {
            set_last_error("scene exceeds the device stacks: transform nesting inside CSG operands " +
                           std::to_string(max_ray_depth) + " (max " + std::to_string(kBigRayStack) +
                           "), CSG operand depth " + std::to_string(max_ivl_depth) + " (max " +
                           std::to_string(kBigIvlSpill + 2) + "), medium.recursion " +
                           std::to_string(d.recursion_limit) + " with reflection/refraction (max " +
                           std::to_string(kBigDepth + 1) + ")");
            return RT_ERR_UNSUPPORTED;
        }
        if (fp32) {
            set_last_error("the FP32 fast path has only the common device stacks; render this scene in FP64");
            return RT_ERR_UNSUPPORTED;
        }
        *big = true;
    }
    return RT_OK;
}
}  // namespace

// ------------------------------------------------------------ kernel variant
int wave_cull_min() {
    static const int v = [] {
        const char* e = std::getenv("RT_WV_MIN");
        return e && *e ? std::max(1, std::atoi(e)) : 4;
    }();
    return v;
}

const char* variant_ns_name(int ns) { return ns == KernelVariant::kRtdb ? "rtdb" : ns == KernelVariant::kRtf ? "rtf" : "rtd"; }

namespace {
// What every pick_* shares.  frames_if_secondary: whether the trace keeps
// reflection / refraction frames (a standard frame or a radiance query: then
// recursion_limit - 1 of them when the scene is secondary).  Sets secondary, ns
// (the stack tier), eager and deep.
int pick_common(const CompiledScene& cs, const rt_scene_desc& d, bool frames_if_secondary, bool fp32, KernelVariant& v) {
    for (int i = 0; i < d.n_materials; ++i)
        if (d.materials[i].kr > 0.0 || d.materials[i].kt > 0.0) v.secondary = true;
    if (d.recursion_limit < 2) v.secondary = false;   // depth < limit-1 never holds (tracer.cpp:38,51)
    bool big = false;
    const int rc = stack_tier(cs.max_ray_depth, cs.max_ivl_depth, d,
                              frames_if_secondary && v.secondary ? d.recursion_limit - 1 : 0, fp32, &big);
    if (rc != RT_OK) return rc;
    v.ns = big ? KernelVariant::kRtdb : fp32 ? KernelVariant::kRtf : KernelVariant::kRtd;
    // the big-stack build has only the general variants (every feature);
    // eager scenes always use D; the lean kernels carry no directional-light
    // code: such scenes take the general (D) variants
    v.eager = big || cs.has_eager;
    v.deep = v.eager || cs.max_ivl_depth > 2 || d.n_dir_lights > 0;
    return RT_OK;
}
// The plain variants: lean (not D) kernels of plain scenes, unless RT_PLAIN=0
bool pick_plain(const CompiledScene& cs, const KernelVariant& v) {
    static const bool plain_on = env_on("RT_PLAIN");
    return !v.deep && plain_on && plain_scene(cs);
}
}  // namespace

int pick_variant(const CompiledScene& cs, const rt_scene_desc& d, int mode, int flags, bool bvh_enabled,
                 KernelVariant* out) {
    KernelVariant v;
    const bool fp32 = (flags & RT_FLAG_FP32) != 0;
    const int rc = pick_common(cs, d, mode == RT_MODE_STANDARD, fp32, v);
    if (rc != RT_OK) return rc;
    v.count_ops = (flags & RT_FLAG_COUNT_OPS) != 0;
    if (!v.deep) {
        int n_bounded = 0;
        for (const auto& o : cs.objs)
            if (o.has_bound && o.kind != OBJ_GROUP) ++n_bounded;
        const bool wave_cull = !(flags & RT_FLAG_NO_CULL) && n_bounded >= wave_cull_min();
        const bool bvh = wave_cull && bvh_enabled && !(flags & RT_FLAG_NO_BVH) && !cs.wchunk.empty();
        v.wv = bvh ? 2 : wave_cull ? 1 : 0;
        // the plain variants: FP64 only, never op-counting; standard-mode
        // reflection / refraction without wave culls runs the general kernel
        // k_std<false, false, true>, which has none
        const bool general = mode == RT_MODE_STANDARD && v.secondary && v.wv == 0;
        v.plain = !general && !fp32 && !v.count_ops && pick_plain(cs, v);
    }
    *out = v;
    return RT_OK;
}

int check_query_flags(int flags) {
    if (flags & RT_FLAG_FP32) {
        set_last_error("ray queries have no FP32 kernels (RT_FLAG_FP32): they run the FP64 parity path");
        return RT_ERR_UNSUPPORTED;
    }
    if (flags & RT_FLAG_COUNT_OPS) {
        set_last_error("ray queries do not count ops (RT_FLAG_COUNT_OPS)");
        return RT_ERR_UNSUPPORTED;
    }
    return RT_OK;
}

int pick_query_variant(const CompiledScene& cs, const rt_scene_desc& d, int flags, KernelVariant* out) {
    int rc = check_query_flags(flags);
    if (rc != RT_OK) return rc;
    KernelVariant v;
    rc = pick_common(cs, d, false, false, v);
    if (rc != RT_OK) return rc;
    v.secondary = false;   // (a query traces one ray)
    v.plain = pick_plain(cs, v);
    *out = v;
    return RT_OK;
}

bool use_ray_bvh(const CompiledScene& cs, const KernelVariant& v, int flags) {
    return (flags & RT_FLAG_RAY_BVH) && !(flags & RT_FLAG_NO_CULL) && !cs.rnodes.empty() && !v.eager &&
           v.ns == KernelVariant::kRtd;
}

int pick_shade_variant(const CompiledScene& cs, const rt_scene_desc& d, int flags, KernelVariant* out) {
    // (shade()'s only scene walk is Scene::occluded: the occluded query's rule)
    return pick_query_variant(cs, d, flags, out);
}

int pick_radiance_variant(const CompiledScene& cs, const rt_scene_desc& d, int flags, KernelVariant* out) {
    int rc = check_query_flags(flags);
    if (rc != RT_OK) return rc;
    KernelVariant v;
    rc = pick_common(cs, d, true, false, v);
    if (rc != RT_OK) return rc;
    if (v.eager) v.secondary = true;   // (the general row: the only eager one)
    v.plain = pick_plain(cs, v);
    *out = v;
    return RT_OK;
}

int pick_node_variant(const rt_scene_desc& d, int node, const NodeProgram& p, int flags, KernelVariant* out) {
    int rc = check_query_flags(flags);
    if (rc != RT_OK) return rc;
    if (node < 0 || node >= d.n_nodes) {
        set_last_error("node index out of range");
        return RT_ERR_INVALID_ARG;
    }
    KernelVariant v;
    const int kind = d.nodes[node].kind;
    if (kind != RT_NODE_SPHERE && kind != RT_NODE_HALFSPACE && kind != RT_NODE_POKEBALL) {
        bool big = false;
        rc = stack_tier(p.max_ray_depth, p.max_ivl_depth, d, 0, false, &big);
        if (rc != RT_OK) return rc;
        v.ns = big ? KernelVariant::kRtdb : KernelVariant::kRtd;
        v.eager = true;
    }
    *out = v;
    return RT_OK;
}

// ----------------------------------------------------------------- dist plan
int strip_height(int mode) { return mode == RT_MODE_PAPER ? RT_PAPER_STRIP_ROWS : RT_STRIP_ROWS; }

int64_t root_shed(int mode) {
    static const int shed_paper = env_int("RT_ROOT_SHED_PAPER", kRootShedPaper);
    static const int shed_std = env_int("RT_ROOT_SHED_STD", kRootShedStd);
    return mode == RT_MODE_PAPER ? shed_paper : shed_std;
}

int frame_chunks(int mode) {
    static const int c[2] = {env_int("RT_DIST_CHUNKS", kChunks), env_int("RT_DIST_CHUNKS_PAPER", kPaperChunks)};
    return std::min(kChunks, std::max(1, c[mode == RT_MODE_PAPER ? 1 : 0]));
}

int paper_chunks_1gpu() {
    static const int c = std::max(1, std::min(4, env_int("RT_PAPER_CHUNKS_1GPU", 1)));
    return c;
}

std::vector<int> strip_owners(int n_strips, int world, int64_t c) {
    std::vector<int> own((size_t)std::max(0, n_strips), 0);
    if (world <= 1) return own;
    std::vector<int64_t> w((size_t)world, 1000), cur((size_t)world, 0);
    w[0] = std::max<int64_t>(500, 1000 - c * world);
    int64_t total = 0;
    for (int64_t v : w) total += v;
    for (int s = 0; s < n_strips; ++s) {
        for (int r = 0; r < world; ++r) cur[r] += w[r];
        const int rot = (s / world) % world;
        int best = rot;
        for (int i = 1; i < world; ++i) {
            const int r = (rot + i) % world;
            if (cur[r] > cur[best]) best = r;
        }
        own[s] = best;
        cur[best] -= total;
    }
    return own;
}

std::vector<std::vector<int32_t>> partition_rows(int H, int world, int mode, int64_t shed) {
    const int S = strip_height(mode);
    const int n_strips = (H + S - 1) / S;
    std::vector<std::vector<int32_t>> rows((size_t)world);
    const std::vector<int> own = strip_owners(n_strips, world, shed);
    for (int st = 0; st < n_strips; ++st)
        for (int r = st * S; r < std::min(H, (st + 1) * S); ++r) rows[own[st]].push_back(r);
    return rows;
}

std::vector<std::pair<int, int>> row_chunks(int m, int chunks, int S) {
    const int64_t units = (m + S - 1) / S;
    chunks = (int)std::max<int64_t>(1, std::min<int64_t>(chunks, units));
    const int64_t wsum = (int64_t)chunks * (chunks + 1) / 2;
    std::vector<std::pair<int, int>> out;
    int64_t acc = 0;
    for (int k = 0; k < chunks; ++k) {
        const int64_t u0 = acc * units / wsum;
        acc += chunks - k;
        const int64_t u1 = acc * units / wsum;
        const int a = (int)std::min<int64_t>(m, u0 * S), b = (int)std::min<int64_t>(m, u1 * S);
        if (b > a) out.emplace_back(a, b);
    }
    if (out.empty()) out.emplace_back(0, 0);
    return out;
}

DistPlan plan_dist_frame(int H, int world, int rank, int mode, int64_t shed, int chunks, bool with_table) {
    DistPlan p;
    const std::vector<std::vector<int32_t>> part = partition_rows(H, world, mode, shed);
    p.rows = part[rank];
    for (const auto& pr : part) p.m = std::max(p.m, (int)pr.size());
    p.bounds = row_chunks(p.m, chunks, strip_height(mode));
    if (with_table) {
        p.rowtab.assign((size_t)world * p.m, -1);
        for (int r = 0; r < world; ++r) {
            const std::vector<int32_t>& rr = part[r];
            for (const auto& ab : p.bounds)
                for (int i = ab.first; i < ab.second; ++i)
                    p.rowtab[(size_t)world * ab.first + (size_t)r * (ab.second - ab.first) + (i - ab.first)] =
                        i < (int)rr.size() ? rr[i] : -1;
        }
    }
    return p;
}

// ------------------------------------------------------- standard-mode plan
StdPlan plan_std_frame(int W, int H, const int32_t* rows, int n_rows, int64_t ckpt_outputs) {
    StdPlan p;
    if (n_rows <= 0) return p;
    const int64_t row_q = (int64_t)32 * W;
    std::vector<int32_t> order(n_rows);
    for (int ri = 0; ri < n_rows; ++ri) order[ri] = ri;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return rows[a] > rows[b]; });
    p.rows_jrow.assign(rows, rows + n_rows);
    p.rows_jrow.resize(2 * (size_t)n_rows);
    for (int k = 0; k < n_rows; ++k) {
        const int ri = order[k];
        p.rows_jrow[n_rows + ri] = k;
        const int64_t y = H - 1 - rows[ri];
        if (!p.jranges.empty() && p.jranges.back().qb == row_q * y)
            p.jranges.back().qb += row_q;
        else
            p.jranges.push_back(JRange{row_q * y, row_q * (y + 1), (int64_t)k * 16 * W});
    }
    // the checkpoint table must reach the last loop row's stream words
    p.q_end = p.jranges.back().qb;
    p.n_ckpt = (p.q_end - 1) / ckpt_outputs + 1;
    return p;
}

// ----------------------------------------------------------- paper-mode plan
uint64_t paper_frame_key(uint64_t uid, int W, int H, int mode, int flags, const int32_t* rows, int n_rows) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](uint64_t v) {
        for (int i = 0; i < 8; ++i) {
            h ^= (v >> (8 * i)) & 0xff;
            h *= 1099511628211ull;
        }
    };
    mix(uid);
    mix((uint64_t)(uint32_t)W << 32 | (uint32_t)H);
    mix((uint64_t)(uint32_t)mode << 32 | (uint32_t)flags);
    mix((uint64_t)n_rows);
    for (int i = 0; i < n_rows; ++i) mix((uint64_t)(uint32_t)rows[i]);
    return h;
}

PaperPlan plan_paper_frame(uint64_t uid, int W, int H, int mode, int flags, const int32_t* rows, int n_rows) {
    PaperPlan p;
    p.W = W;
    p.H = H;
    p.n_rows = n_rows;
    p.rows.assign(rows, rows + n_rows);
    std::vector<char> need(H, 0), shade_row(H, 0);
    for (int r : p.rows) {
        need[r] = 1;
        shade_row[r] = 1;
        if (r > 0) need[r - 1] = 1;
        if (r + 1 < H) need[r + 1] = 1;
    }
    std::vector<int32_t> ext, ext_shade;
    p.ext_pos.assign(H, -1);
    for (int r = 0; r < H; ++r)
        if (need[r]) {
            p.ext_pos[r] = (int)ext.size();
            ext.push_back(r);
            ext_shade.push_back(shade_row[r]);
        }
    p.n_ext = (int)ext.size();
    std::vector<int32_t> nbr(3 * (size_t)n_rows);
    for (int i = 0; i < n_rows; ++i) {
        const int r = p.rows[i];
        nbr[3 * i + 0] = r > 0 ? p.ext_pos[r - 1] : -1;
        nbr[3 * i + 1] = p.ext_pos[r];
        nbr[3 * i + 2] = r + 1 < H ? p.ext_pos[r + 1] : -1;
        p.logical_isect += (uint64_t)W * 2 + (uint64_t)(W > 1 ? 2 * (W - 1) : 0) +
                           (uint64_t)W * ((r > 0) + (r + 1 < H));
    }
    p.aux.reserve(p.off_lists());
    p.aux.insert(p.aux.end(), ext.begin(), ext.end());
    p.aux.insert(p.aux.end(), ext_shade.begin(), ext_shade.end());
    p.aux.insert(p.aux.end(), nbr.begin(), nbr.end());
    p.aux.insert(p.aux.end(), p.rows.begin(), p.rows.end());
    p.key = paper_frame_key(uid, W, H, mode, flags, rows, n_rows);
    return p;
}

void order_paper_groups(std::vector<int32_t>& list, const std::vector<uint32_t>* cost) {
    if (!cost) return;
    const size_t nb = list.size() / 16;
    std::vector<std::pair<uint64_t, size_t>> key(nb);
    for (size_t b = 0; b < nb; ++b) {
        uint64_t c = 0;
        for (size_t g = 2 * b; g < 2 * b + 2; ++g) {
            int32_t e = -1;
            for (size_t i = 0; i < 8 && e < 0; ++i) e = list[8 * g + i];
            if (e < 0) continue;
            if ((size_t)e >= cost->size() || (*cost)[e] == 0) return;   // not measured: row order
            c += (*cost)[e];
        }
        key[b] = {c, b};
    }
    std::stable_sort(key.begin(), key.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    std::vector<int32_t> out(list.size());
    for (size_t j = 0; j < nb; ++j) std::copy_n(list.begin() + 16 * key[j].second, 16, out.begin() + 16 * j);
    list.swap(out);
}

const std::vector<int32_t> PaperCalls::kEmpty;

void PaperCalls::reset(const PaperPlan* plan) {
    plan_ = plan;
    ext_done_.assign(plan ? plan->n_ext : 0, 0);
    stream_.clear();
    marked_.clear();
    lists_.clear();
    list_used_ = 0;
}

PaperCalls::Call PaperCalls::next_call(int ri0, int ri1, uintptr_t stream_id, const std::vector<uint32_t>* cost) {
    const PaperPlan& p = *plan_;
    Call c;
    // A call whose finish pass reads primary hits that an earlier call
    // computed on another stream waits for that call's primary pass (adjacent
    // strips share a neighbour row)
    std::vector<char> wait(stream_.size(), 0);
    std::vector<int32_t> list;
    marked_.clear();
    int prev_row = -2;
    for (int i = ri0; i < ri1; ++i) {
        const int r = p.rows[i];
        for (int rr = r - 1; rr <= r + 1; ++rr) {
            if (rr < 0 || rr >= p.H) continue;
            const int e = p.ext_pos[rr];
            if (e < 0) continue;
            if (ext_done_[e] && ext_done_[e] <= n_calls()) {   // an earlier call computed it
                if (stream_[ext_done_[e] - 1] != stream_id) wait[ext_done_[e] - 1] = 1;
            } else if (!ext_done_[e]) {
                ext_done_[e] = n_calls() + 1;   // (this call's index + 1)
                marked_.push_back(e);
                if (rr != prev_row + 1)
                    while (list.size() % 8) list.push_back(-1);
                list.push_back(e);
                prev_row = rr;
            }
        }
    }
    while (list.size() % 16) list.push_back(-1);
    if ((size_t)list_used_ + list.size() > p.list_cap()) {
        for (int32_t e : marked_) ext_done_[e] = 0;
        marked_.clear();
        return c;
    }
    for (size_t k = 0; k < wait.size(); ++k)
        if (wait[k]) c.wait.push_back((int)k);
    stream_.push_back(stream_id);
    c.ok = true;
    c.list = &kEmpty;
    c.list_off = list_used_;
    if (!list.empty()) {
        order_paper_groups(list, cost);
        lists_.push_back(Launched{list_used_, std::move(list)});
        list_used_ += (int)lists_.back().list.size();
        c.list = &lists_.back().list;
    }
    return c;
}

void PaperCalls::rollback() {
    for (int32_t e : marked_) ext_done_[e] = 0;
    marked_.clear();
    if (!stream_.empty()) stream_.pop_back();
}

void PaperCalls::group_costs(const uint32_t* gc, std::vector<uint32_t>& cost) const {
    cost.resize(plan_->n_ext, 0);
    for (const Launched& c : lists_)
        for (size_t g = 0; g < c.list.size() / 8; ++g) {
            int32_t e = -1;
            for (size_t i = 0; i < 8 && e < 0; ++i) e = c.list[8 * g + i];
            if (e >= 0) cost[e] = std::max(1u, gc[c.list_off / 8 + g]);
        }
}

}  // namespace rtamd
