// frame_plan.hpp — a frame's decisions as host-only integer logic (no HIP).
//
// Which trace kernel a frame launches (pick_variant), which rows a rank owns,
// how they are chunked and where a gathered slot lands (plan_dist_frame), the
// standard-mode jitter layout (plan_std_frame) and the paper-mode halo rows,
// buffer layout and per-call lists (plan_paper_frame, PaperCalls).
// rt_frame.hip and rt_dist.hip execute these plans; tests/test_frame_plan.py
// checks them on the CPU through the rt_test_plan_* hooks and
// tools/sanitize/host_check.cpp runs them under ASan/UBSan.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "rt.h"
#include "scene_compile.hpp"

namespace rtamd {

// ------------------------------------------------------------ kernel variant
// Per-lane stacks of the render kernels (checked on the host per scene).
// The common kernels carry small ones; scenes beyond them run on the
// "big-stack" build of the general kernels (namespace rtdb,
// rt_kernels_big.hip), whose stacks live in scratch memory.
constexpr int kMaxRayStack = 8;   // transform nesting inside CSG operands (eager programs)
constexpr int kMaxIvlSpill = 6;   // CSG interval stack entries beyond the top two
constexpr int kMaxDepth = 16;     // reflection/refraction frames (medium.recursion <= 17)
constexpr int kBigRayStack = 64;
constexpr int kBigIvlSpill = 62;
constexpr int kBigDepth = 128;    // medium.recursion <= 129

// Scenes with at least this many bounded objects take the wave-level culling
// kernels (wv >= 1).  RT_WV_MIN overrides it (measurement A/B; default 4).
int wave_cull_min();

// One trace kernel: the key of the dispatch tables of rt_kernels.hpp.  Always
// canonical: wv and plain are 0 / false where the kernel has no such build
// (the general kernels k_std / k_paper_primary).  secondary is the scene's in
// either mode (the paper kernels have no SEC and ignore it), timed is set per
// paper-mode launch.
struct KernelVariant {
    enum Ns { kRtd = 0, kRtf = 1, kRtdb = 2 };   // FP64 parity, FP32 (RT_FLAG_FP32), FP64 big-stack
    int ns = kRtd;
    bool eager = false;       // E: the scene has eager (transform inside CSG operand) objects
    bool deep = false;        // D: general compact CSG (deep stacks, directional lights)
    bool secondary = false;   // SEC: reflection / refraction frames
    bool count_ops = false;   // C: RT_FLAG_COUNT_OPS
    bool plain = false;       // PL: only sphere / half-space / pokeball objects (CntPlain, rt_device.hpp)
    int wv = 0;               // WV: 0 per-lane culls, 1 wave-level culls, 2 wave BVH
    bool timed = false;       // T: a paper-mode launch that stores its waves' ticks (set per launch)
};
const char* variant_ns_name(int ns);   // "rtd" / "rtf" / "rtdb"

// The variant a frame of (scene, mode, flags) launches.  bvh_enabled: false
// when the frame's BVH trial (rt_workspace.hpp SceneCache) runs it without the
// wave BVH.  RT_OK, or RT_ERR_UNSUPPORTED with the message set: a scene
// beyond the big stacks, or beyond the common ones in FP32.
int pick_variant(const CompiledScene& cs, const rt_scene_desc& d, int mode, int flags, bool bvh_enabled,
                 KernelVariant* out);

// The variant a ray query (rt_query_intersect / rt_query_occluded) of (scene,
// flags) launches: pick_variant's stack tiers (no recursion frames: a query
// traces one ray) and its eager / deep / plain rules, always with per-lane
// culls (wv = 0: a query's rays are arbitrary, the wave-level culls and the
// wave BVH bound a pixel tile's) and never secondary.  RT_OK, or
// RT_ERR_UNSUPPORTED with the message set: RT_FLAG_FP32 or RT_FLAG_COUNT_OPS
// (queries are FP64 and uncounted: check_query_flags, which a query asks
// before anything else), or a scene beyond the big stacks.
int check_query_flags(int flags);
int pick_query_variant(const CompiledScene& cs, const rt_scene_desc& d, int flags, KernelVariant* out);
// Whether a ray query of variant v (pick_query_variant's) launches the ray-BVH
// row of (D, PL) (rt_query_bvh_kernels.hpp) instead of the flat one:
// RT_FLAG_RAY_BVH without RT_FLAG_NO_CULL, a scene with a ray BVH (it has a
// wave list: more than kWaveBvhMin objects, no eager programs) and the
// namespace rtd.  In every other case the flag is accepted and changes nothing.
bool use_ray_bvh(const CompiledScene& cs, const KernelVariant& v, int flags);

// The variant a shading query (rt_query_shade: shade_lambert_phong of
// caller-given hits) of (scene, flags) launches: pick_query_variant's rule, as
// the kernel's scene walks are the shadow rays' Scene::occluded calls (E, D,
// PL and the stack tier of a query without recursion frames; D also carries
// the directional lights' code).  Looked up in the shade tables (rt_launch.hpp
// KernelNamespace::shade).
int pick_shade_variant(const CompiledScene& cs, const rt_scene_desc& d, int flags, KernelVariant* out);

// The variant a radiance query (rt_query_radiance: Tracer::trace of caller-given
// rays) of (scene, flags) launches: check_query_flags first, then
// pick_variant's standard-mode rules with per-lane culls forced (wv = 0, as
// for the other queries).  secondary is the frame's, and the stack tiers count
// the frame's recursion frames (recursion_limit - 1 when secondary), so a
// scene whose frames need the big stacks takes them here too.  Eager scenes
// (and every big-stack one) take the general kernel with secondary set
// whatever the materials say: its loop never descends without a reflecting or
// refracting hit, and the radiance table has no other eager row.
int pick_radiance_variant(const CompiledScene& cs, const rt_scene_desc& d, int flags, KernelVariant* out);

// The variant a node query (rt_query_node_intersect / rt_query_node_interval)
// of node `node` of d launches, looked up in the node tables (rt_launch.hpp
// KernelNamespace::node): check_query_flags first; a sphere, half-space or
// pokeball node takes the leaf row (eager = false: no interpreter, no stacks,
// namespace rtd whatever the scene); any other node the program row (eager =
// true) of the stack tier of ITS OWN program p (compile_node_program), not the
// scene's: rtd within kMaxRayStack / kMaxIvlSpill + 2, rtdb up to kBigRayStack
// / kBigIvlSpill + 2, beyond that RT_ERR_UNSUPPORTED with the frames' message.
// The per-lane stacks are fixed arrays, so that refusal is what keeps a deeper
// program from ever reaching the device.  Only ns and eager are set.
int pick_node_variant(const rt_scene_desc& d, int node, const NodeProgram& p, int flags, KernelVariant* out);

// ----------------------------------------------------------------- dist plan
constexpr int kChunks = 4;   // pipeline units per rank (chunk k gathered while k+1 is traced)
// Paper frames gather one code byte per pixel, so their chunks hide little
// transfer, while every chunk adds a launch tail of the costly paper waves:
// 2 chunks project config 5 at 8 ranks 5.21-5.23x -> 5.46-5.56x, at 4 ranks
// 3.04 -> 3.12-3.18x (1: 4.58x, 3: 5.30x; profiles/r06_ab/ab_dist_chunks.txt).
constexpr int kPaperChunks = 2;
// The root's strip shed per mille and rank (strip_owners)
constexpr int kRootShedPaper = 45, kRootShedStd = 8;

// Strip height per mode: standard mode RT_STRIP_ROWS (8); paper mode
// RT_PAPER_STRIP_ROWS (30): each strip's primary hits are traced with its two
// neighbour rows (the edge probes, tracer.cpp:133-178), and 30 + 2 = 32 rows
// keep every 8-row wave of k_paper_primary inside one strip (coherent rays
// for the wave-level culls) at 1/15 halo overhead (8-row strips: 1/4 extra
// rows and waves straddling strips 16+ rows apart).
int strip_height(int mode);
// (RT_ROOT_SHED_PAPER / RT_ROOT_SHED_STD: measurement A/B only.  Both values
// travel in the frame descriptor, so ranks that see different ones refuse the
// frame together instead of tracing another partition than the root places.)
int64_t root_shed(int mode);
// Row chunks per rank and frame (each one gather): kChunks (paper: kPaperChunks), or
// RT_DIST_CHUNKS (standard mode) / RT_DIST_CHUNKS_PAPER from the environment
// (measurement A/B; 1 .. kChunks).
int frame_chunks(int mode);
// RT_PAPER_CHUNKS_1GPU (measurement A/B; 1 .. 4, default 1): row chunks of a
// paper frame rendered by one GPU, alternating between two streams so that
// chunk k's finish pass overlaps chunk k+1's primary.  Measured on config 5
// (profiles/r05_ab/ab_paper_chunks_1gpu.txt): 1 chunk 5.34 ms, 2 chunks 5.37,
// 4 chunks 5.57 - the chunks' own tails and their separate costliest-first
// orders cost more than the overlapped finish saves - so one launch pair.
int paper_chunks_1gpu();

// Which rank renders strip s.  Interleaved so that every rank samples the
// whole frame (cheap sky rows against expensive geometry rows), by a smooth
// weighted round robin: every strip, each rank's credit grows by its weight
// and the rank with the most credit takes the strip (and pays the total).
//  * Ties go to the rank first in a per-round rotation (round k = strips
//    [k*world, (k+1)*world) starts at rank k mod world), so a rank's strips do
//    not all sit at the same phase of a world*S-row period: config 5's sphere
//    rows have structure on that scale (a plain s mod world split left the
//    slowest of 8 paper-mode ranks 11 % above the mean).
//  * Rank 0 also places every gathered strip into the frame (the FP64 frame:
//    24 B/px written; paper mode decodes one byte per pixel into 24), so it
//    renders fewer strips: weight 1 - c*world (per mille: c = 45 paper, 8
//    standard, 0 for RGB8 output; from per-rank timings, profiles/r04*; the
//    paper value raised 30 -> 45 with the plain paper kernel, whose faster
//    trace left the root's placement the longest leg: 8-rank frame
//    0.726 -> 0.708 ms, profiles/r06_ab/ab_dist_shed_plain.txt).
// The partition is a pure function of (H, world, mode, kind), all of which
// the ranks check against each other before the first gather.
std::vector<int> strip_owners(int n_strips, int world, int64_t c);
// Output rows of every rank (ascending per rank), strips of strip_height(mode).
// (A partition balanced on measured strip costs - the strips' summed primary
// wave ticks, exchanged in the trace-status agreement, longest processing
// time first - was measured and rejected: slower at 2 ranks, no better at 4
// and 8, profiles/r05_ab/ab_cost_partition.txt.)
// shed: the root's per-mille shed for this frame (0 for RGB8 output; else
// root_shed(mode), which every rank checks in the frame descriptor).
std::vector<std::vector<int32_t>> partition_rows(int H, int world, int mode, int64_t shed);
// `chunks` contiguous pieces of [0, m), each a whole number of strips of S
// rows (a chunk never splits a strip, so a paper-mode strip's rows and halo
// are traced by one launch), of decreasing size (weights chunks, chunks-1,
// ..., 1: 4 chunks = 40/30/20/10 %).  Chunk k is gathered while chunk k+1 is
// traced, so only the last, smallest chunk's gather is exposed.
std::vector<std::pair<int, int>> row_chunks(int m, int chunks, int S = 1);

// One rank's part of a distributed frame.
struct DistPlan {
    std::vector<int32_t> rows;                  // the rank's output rows (ascending; may be empty)
    int m = 0;                                  // rows of the fullest rank: every rank's padded list length
    std::vector<std::pair<int, int>> bounds;    // row chunks of [0, m)
    // the root's placement table (with_table): chunk [a, b) occupies slots
    // [world*a, world*b) as [rank][b-a], so slot world*a + r*(b-a) + (i-a)
    // holds rank r's i-th row (-1: padding)
    std::vector<int32_t> rowtab;
};
DistPlan plan_dist_frame(int H, int world, int rank, int mode, int64_t shed, int chunks, bool with_table);

// ------------------------------------------------------- standard-mode plan
// A run of stream outputs: the draw made of outputs q, q+1 (q even, in
// [qa, qb)) is stored at jit[dst + (q - qa)/2].  Ranges passed to the
// launcher are sorted by qa and disjoint.  A rendered loop row y of width W
// is the range [32*W*y, 32*W*(y+1)) (tracer.cpp:284-293: 8 samples x 2
// draws x 2 words).
struct JRange {
    int64_t qa, qb, dst;
};

// Loop row y = H-1-rows[ri] consumes outputs [32Wy, 32W(y+1))
// (tracer.cpp:284-293).  Jitter rows are laid out in stream order (jrow =
// rank of y), so runs of consecutive loop rows - a strip, or the whole
// frame - are one range for the generator.
struct StdPlan {
    std::vector<int32_t> rows_jrow;   // rows | jitter row of each
    std::vector<JRange> jranges;      // coalesced, ascending
    int64_t q_end = 0;                // one past the last stream output any row reads
    int64_t n_ckpt = 0;               // checkpoints the table needs to reach it (one per ckpt_outputs)
};
StdPlan plan_std_frame(int W, int H, const int32_t* rows, int n_rows, int64_t ckpt_outputs);

// ----------------------------------------------------------- paper-mode plan
// primary waves per 8-entry list group (k_paper_primary: 16-column blocks of 2x2 waves)
inline int paper_waves_per_group(int W) { return 2 * ((W + 15) / 16); }
// Workspace::paper_cost key of a frame (scene, size, mode, flags, rows)
uint64_t paper_frame_key(uint64_t uid, int W, int H, int mode, int flags, const int32_t* rows, int n_rows);

// ext = the rows needing a primary hit: rendered rows and their vertical
// neighbours.  aux is the device buffer's fixed head,
//   ext_rows[n_ext] | ext_shade[n_ext] | nbr[3*n_rows] | rows[n_rows]
// followed by list_cap entries for the trace calls' ext lists (every ext entry
// once, each run padded by < 8 to a group boundary and each call's list by
// < 16 to a block).
struct PaperPlan {
    int W = 0, H = 0, n_rows = 0, n_ext = 0;
    std::vector<int32_t> rows;
    std::vector<int32_t> ext_pos;   // output row -> ext index (-1: none)
    std::vector<int32_t> aux;
    uint64_t logical_isect = 0;     // Scene::intersect calls: trace_paper + centre + valid neighbours
    uint64_t key = 0;
    size_t off_ext_rows() const { return 0; }
    size_t off_ext_shade() const { return (size_t)n_ext; }
    size_t off_nbr() const { return 2 * (size_t)n_ext; }
    size_t off_rows() const { return 2 * (size_t)n_ext + 3 * (size_t)n_rows; }
    size_t off_lists() const { return 2 * (size_t)n_ext + 4 * (size_t)n_rows; }
    size_t list_cap() const { return 24 * (size_t)n_ext; }
    size_t aux_ints() const { return off_lists() + list_cap(); }
    // primary waves' (start, end) ticks: <= 3 list groups per ext row (the
    // list capacity / 8), paper_waves_per_group waves per group
    size_t gtime_words() const { return (size_t)3 * n_ext * paper_waves_per_group(W) * 2; }
};
PaperPlan plan_paper_frame(uint64_t uid, int W, int H, int mode, int flags, const int32_t* rows, int n_rows);

// Paper mode launch order.  A wave of k_paper_primary covers one 8-entry
// group of the ext list; a group's cost varies ~10x over a frame (sky rows
// against crowded ones, profiles/r04s_strips5.json).  Launched in row order,
// the costly rows of the lower frame start last and their waves form the
// launch's tail: one launch of a rank's rows of an 8-way config-5 frame took
// 0.858 ms in row order, 0.799 ms costliest strips first, 0.994 ms cheapest
// first (profiles/r04y_order5.jsonl).  So every primary wave stores its
// start and end ticks (PaperParams::gtime), rt_frame_end sums them per group
// and keeps them per frame key, and the next frame of that key launches its
// 16-entry blocks (workgroup rows) costliest first.  Measured: one GPU
// 5.37 -> 5.33 ms, the slowest of 8 ranks' trace 0.95 -> 0.93 ms
// (profiles/r04_ab/ab_order.jsonl).  Groups keep their entries (each wave
// stays on 8 consecutive rows of one strip); only the launch order changes,
// which no pixel depends on.  A frame with no history runs in row order.
//
// Reorders the 16-entry blocks of list (one workgroup row: its four waves
// share the workgroup's culls, so a block stays one piece) costliest first
// when every 8-entry group with an entry has a measured cost (else leaves the
// row order); padding blocks go last.
void order_paper_groups(std::vector<int32_t>& list, const std::vector<uint32_t>* cost);

// The trace calls of one paper frame: which ext rows each call's primary pass
// computes (those its rows read that no earlier call computed), and which
// earlier calls' primary passes its finish pass has to wait for.  Streams are
// opaque ids.
class PaperCalls {
public:
    struct Call {
        bool ok = false;                       // false: the lists overflowed their capacity (nothing was marked)
        const std::vector<int32_t>* list = nullptr;   // ext indices, -1 padding; empty: nothing left to compute
        int list_off = 0;                      // its offset behind PaperPlan::off_lists()
        std::vector<int> wait;                 // earlier calls on another stream whose primary hits it reads
    };
    void reset(const PaperPlan* plan);
    // k_paper_primary's waves are 8 list entries tall: each run of consecutive
    // rows starts on a wave boundary (entries -1 pad), so no wave mixes rows of
    // different strips (the wave-level culls need coherent rays); the list is
    // padded to whole 16-entry blocks (the group index is li / 8) and, given
    // cost, ordered by order_paper_groups.
    Call next_call(int ri0, int ri1, uintptr_t stream_id, const std::vector<uint32_t>* cost = nullptr);
    // The last next_call failed before its events were recorded: its ext
    // entries are unmarked and its stream record dropped, so that a later call
    // never waits on it.  (Its list space stays consumed: its upload may be queued.)
    void rollback();
    int n_calls() const { return (int)stream_.size(); }
    uintptr_t stream_of(int call) const { return stream_[call]; }
    int list_used() const { return list_used_; }   // a multiple of 16
    const std::vector<int>& ext_done() const { return ext_done_; }
    // This frame's group costs by each group's first ext index, from the
    // reduced wave times gc[list_used / 8] (0 ticks count as 1: measured).
    void group_costs(const uint32_t* gc, std::vector<uint32_t>& cost) const;

private:
    const PaperPlan* plan_ = nullptr;
    std::vector<int> ext_done_;          // primary hit launched by call (value - 1); 0 = not yet
    std::vector<uintptr_t> stream_;      // stream of each call
    std::vector<int32_t> marked_;        // ext entries of the last call
    int list_used_ = 0;
    struct Launched {
        int list_off;
        std::vector<int32_t> list;       // (also the host source of its async upload)
    };
    std::vector<Launched> lists_;
    static const std::vector<int32_t> kEmpty;
};

}  // namespace rtamd
