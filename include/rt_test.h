/*
 * rt_test.h — test hooks exported by librtamd.so (not part of the drop-in
 * boundary; used by tests/ to check the jitter-stream machinery in isolation).
 */
#ifndef RT_TEST_H
#define RT_TEST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* CPU check of the GF(2) jump polynomials (csrc/host/mt_poly.cpp): for
 * tree levels j < levels and m = 1..7, applying x^(624*K*m*8^j) mod phi to
 * the seed window must equal advancing it m*8^j*K twist blocks
 * sequentially.  Returns the number of mismatching polynomials (0 = all
 * good), -1 on error. */
int rt_test_mt_jump_cpu(int K_blocks, int levels);

/* GPU: generate the jitter stream for output indices [q0, q1) (even) with the
 * device jump/fill kernels at segment length K_blocks twist blocks and copy
 * uniform draws [first, first+count) (draw index = output index / 2) to
 * out_host.  K_blocks == 0 selects the frame path instead: the resident
 * checkpoint table (every 64 twist blocks, built by the same jump tree) and
 * the one-wavefront fill kernel.  Returns an rt_status. */
int rt_test_jitter_device(int K_blocks, int64_t q0, int64_t q1, int64_t first, int64_t count, double* out_host);

/* Host-only: compile a scene to its device object table and report
 * out[8] = {objects incl. cull headers, object cull groups, their members,
 * program ops, CSG operand groups (OP_IVL_GROUP), their members, has eager
 * programs, max CSG operand depth}.  No device is touched. */
struct rt_scene;
int rt_test_compile_info(const struct rt_scene* s, int32_t* out);

/* Host-only: a histogram of the compiled forms of a scene (scene_compile.hpp),
 * which rt_test_compile_info's totals do not tell apart, into
 * out[0 .. RT_TEST_FORMS_LEN) (cap >= RT_TEST_FORMS_LEN), at these offsets:
 *   OBJ + k          objects of DevObjKind k (7 kinds, cull headers included)
 *   CHAIN_CORE + c   OBJ_CHAIN objects with a leaf (0) / compact CSG (1) core
 *   CHAIN_M + m      OBJ_CHAIN objects under m = 0, 1, 2, >= 3 transforms
 *   CHAIN_M3_CORE + c  those with m >= 3, by core
 *   FOLD + op        fold objects (DevObj::nfold > 0) per rt_csg_op
 *   OP + k           program ops of DevOpCode k (9 codes)
 *   NEVER_TOP + t    OP_NEVER ops with top = t (0, 1: hit mode; 2: interval mode)
 *   IVL_GROUP + op   OP_IVL_GROUP headers per rt_csg_op
 *   RAY_DEPTH, IVL_DEPTH  CompiledScene::max_ray_depth / max_ivl_depth
 *   BOUNDED          objects (cull headers aside) with a bounding ball
 *   PREFILTER        OBJ_CHAIN objects with leaf prefilter balls
 * No device is touched. */
enum {
    RT_TEST_FORMS_OBJ = 0,
    RT_TEST_FORMS_CHAIN_CORE = 7,
    RT_TEST_FORMS_CHAIN_M = 9,
    RT_TEST_FORMS_CHAIN_M3_CORE = 13,
    RT_TEST_FORMS_FOLD = 15,
    RT_TEST_FORMS_OP = 18,
    RT_TEST_FORMS_NEVER_TOP = 27,
    RT_TEST_FORMS_IVL_GROUP = 30,
    RT_TEST_FORMS_RAY_DEPTH = 33,
    RT_TEST_FORMS_IVL_DEPTH = 34,
    RT_TEST_FORMS_BOUNDED = 35,
    RT_TEST_FORMS_PREFILTER = 36,
    RT_TEST_FORMS_LEN = 37
};
int rt_test_compile_forms(const struct rt_scene* s, int32_t* out, int cap);

/* Host-only: the wave BVH of a scene (CompiledScene::wobjs ...).  counts[2] =
 * {objects in the wave list, chunks} (both 0: no BVH); up to cap_objs
 * entries of worig (each listed object's index in the compiled object table)
 * and of wctab (8 floats per object: its cull record), up to cap_chunks
 * chunk records (8 floats each). */
int rt_test_wave_bvh(const struct rt_scene* s, int32_t* counts, int32_t* worig, float* wctab, int cap_objs,
                     float* wchunk, int cap_chunks);

/* Host-only: the ray BVH of a scene (RT_FLAG_RAY_BVH; CompiledScene::rnodes).
 * counts[3] = {nodes, unbounded lead objects of the wave list (outside the
 * tree: every ray evaluates them), objects in the wave list}; nodes 0: no tree.
 * Up to cap nodes go to nodes_out, 32 bytes each: the f32 ball (cx, cy, cz, r),
 * then int32 skip (the next node in depth-first pre-order when the subtree is
 * culled; the node count at the end), first, count (a leaf's range of the
 * wave list; an inner node has count 0) and a pad word. */
int rt_test_ray_bvh(const struct rt_scene* s, int32_t* counts, void* nodes_out, int cap);
/* Host-only: the kernels' walk restated on the host.  For each ray's fixed
 * segment [tmin, tmax], cand_out[i * n_objects + k] = 1 for every top-level
 * object k (an index into rt_scene_desc.objects) whose evaluation the walk
 * reaches, else 0, and tests_out[i] = the ray's number of node tests (either
 * may be NULL).  RT_ERR_UNSUPPORTED: the scene has no tree. */
int rt_test_ray_bvh_walk(const struct rt_scene* s, const struct rt_ray* rays, size_t n, uint8_t* cand_out,
                         int32_t* tests_out);
/* The kernel ("ns::name") a ray query of kind 0 (intersect) / 1 (occluded) with
 * these flags launches when RT_FLAG_RAY_BVH may be among them: the ray-BVH
 * row where the flag takes effect (frame_plan.hpp use_ray_bvh), else the flat
 * row rt_test_query_kernel_name reports; and row `index` of the ray-BVH table
 * (rtd only).  Host only. */
int rt_test_ray_bvh_kernel_name(const struct rt_scene* s, int kind, int flags, char* out, int cap);
int rt_test_ray_bvh_row(int index, char* out, int cap);

/* Resources of the trace kernel rt_render would launch for this scene, mode
 * and flags (hipFuncGetAttributes + occupancy query): out[8] = {VGPRs per
 * lane, scratch bytes per lane, LDS bytes per workgroup (static + the
 * dynamic shading pool of 10 KiB per wave), resident
 * workgroups per CU, waves per SIMD, max threads per block, wave-level
 * culling variant, reflection/refraction variant}.  Needs a device. */
int rt_test_kernel_info(const struct rt_scene* s, int mode, int flags, int32_t* out);

/* The name of that kernel as rocprofv3 reports it (e.g. "rtd::k_std_lean<false, 1, false>"),
 * NUL-terminated into out[0 .. cap): the frame's own kernel choice
 * (frame_plan.hpp pick_variant) looked up in the launch tables, so a scene a
 * frame refuses (RT_ERR_UNSUPPORTED) is refused here too.  Host only. */
int rt_test_kernel_name(const struct rt_scene* s, int mode, int flags, char* out, int cap);

/* The same for a ray query (rt_query_intersect / rt_query_occluded): kind 0 the
 * closest-hit kernel, 1 the any-hit one (e.g. "rtd::k_query_isect<false, false,
 * true>"): the query's own kernel choice (frame_plan.hpp pick_query_variant)
 * looked up in the query table, so the flags and scenes a query refuses are
 * refused here too.  Host only. */
int rt_test_query_kernel_name(const struct rt_scene* s, int kind, int flags, char* out, int cap);

/* The same for a radiance query (rt_query_radiance; e.g. "rtd::k_radiance<false,
 * false, true, true>"): frame_plan.hpp pick_radiance_variant looked up in the
 * radiance table.  Host only. */
int rt_test_radiance_kernel_name(const struct rt_scene* s, int flags, char* out, int cap);
/* Row `index` of the radiance launch table `table` (0 rtd, 1 rtdb), as
 * rt_test_kernel_row below reads the other tables: "ns::name" into out;
 * RT_OK, or RT_ERR_INVALID_ARG past the end or for another table.  Host only. */
int rt_test_radiance_kernel_row(int table, int index, char* out, int cap);

/* The same pair for a shading query (rt_query_shade; e.g. "rtd::k_shade<false,
 * false, true>"): frame_plan.hpp pick_shade_variant looked up in the shade
 * table, and row `index` of shade launch table `table` (0 rtd, 1 rtdb).  Host
 * only. */
int rt_test_shade_kernel_name(const struct rt_scene* s, int flags, char* out, int cap);
int rt_test_shade_kernel_row(int table, int index, char* out, int cap);

/* The same for a node query (rt_query_node_intersect / rt_query_node_interval)
 * of node `node`: kind 0 the intersect kernel, 1 the interval one (e.g.
 * "rtdb::k_node_ivl<true>"): the query's own choice (compile_node_program +
 * frame_plan.hpp pick_node_variant) looked up in the node table, so the nodes
 * and flags a query refuses are refused here too; and row `index` of node
 * launch table `table` (0 rtd, 1 rtdb).  Host only. */
int rt_test_node_kernel_name(const struct rt_scene* s, int node, int kind, int flags, char* out, int cap);
int rt_test_node_kernel_row(int table, int index, char* out, int cap);
/* That node's own program (scene_compile.hpp compile_node_program): returns
 * its op count (<0: an rt_status) and writes (op, node, top, csg_op) of the
 * first min(count, cap) ops to ops_out[4 * i ..] (ops_out may be NULL with
 * cap 0) and, when depths_out2 is set, {max_ray_depth, max_ivl_depth} of the
 * program itself.  Host only. */
int rt_test_node_program(const struct rt_scene* s, int node, int kind, int32_t* ops_out, int cap, int32_t* depths_out2);

/* The launch log: which kernels ran.  rt_test_kernel_name above is the plan
 * for a frame whose wave BVH is on and untimed; the frame itself may drop the
 * BVH (its trial frames) or launch the timed build of a paper kernel (the
 * first frame of a scene and shape).  The log records what the launchers of
 * rt_kernels.hpp / rt_query_kernels.hpp / rt_radiance_kernels.hpp /
 * rt_shade_kernels.hpp / rt_node_kernels.hpp were asked for, host side only.
 * on != 0: clear the log and start recording; 0: stop.  Process-wide,
 * thread-safe; while recording is off a launch pays one relaxed atomic load. */
int rt_test_launch_log(int on);
/* The kernels launched since recording started, in launch order, one
 * "ns::name" per line (the table row's own name string; finish kernels as
 * "ns::k_paper_finish<CODES, PAIR>"; query kernels likewise), NUL-terminated
 * into out[0..cap).  Returns the number of launches recorded, <0 on error
 * (RT_ERR_INVALID_ARG: cap too small). */
int rt_test_launch_log_get(char* out, int cap);

/* Row `index` of launch table `table`: 0 rtd std, 1 rtd paper, 2 rtf std,
 * 3 rtf paper, 4 rtdb std, 5 rtdb paper, 6 rtd query, 7 rtdb query,
 * 8 finish kernels (rtd's, then rtf's: big-stack frames finish with rtd's).
 * Read from the tables the launchers search, so a build's ifdefs are
 * honoured.  "ns::name" into out; returns RT_OK, or RT_ERR_INVALID_ARG past
 * the end.  Host only. */
int rt_test_kernel_row(int table, int index, char* out, int cap);

/* GPU: the shared-denominator division of the device code (rt_device.hpp
 * div3) next to the compiler's own division on the same inputs:
 * div3_host[3i+k] and plain_host[3i+k] = a[3i+k] / b[i].  Tests require the
 * two to be bit-identical. */
int rt_test_div3(const double* a_host, const double* b_host, int n, double* div3_host, double* plain_host);

/* GPU: the fused square root + division of the device code (rt_device.hpp
 * norm3) next to the compiler's own operations on the same vectors, one lane
 * per vector v_host[3i..3i+2], 256-thread blocks in input order (so the caller
 * decides which vectors share a wave).  L_host[i], q_host[3i+k]: norm3's |v|
 * and v[k] / |v|; plainL_host, plainq_host: __builtin_sqrt of the same sum of
 * squares and `/` in the same kernel; fast_host[i] = 1 if lane i's wave took
 * the fused path (every lane of the wave in range), 0 if it took sqrt + div3.
 * Tests require norm3 and plain to be bit-identical.  Returns an rt_status. */
int rt_test_norm3(const double* v_host, int n, double* L_host, double* q_host, double* plainL_host,
                  double* plainq_host, int* fast_host);

/* GPU: out_host[3i..3i+2] = normalized(v_host[3i..3i+2]) (Dir3::normalized:
 * v / |v|, or (0, 1, 0) when |v| <= 1e-6), launched like rt_test_norm3. */
int rt_test_normalized(const double* v_host, int n, double* out_host);

/* GPU: out_host[i] = pow_spec(x_host[i], y_host[i]), the device code's own
 * std::pow(rdotv, shininess) of the specular term (rt_device.hpp pow_spec,
 * shading.cpp:124), one lane per element, 256-thread blocks in input order (so
 * the caller decides which exponents share a wave).  Contract: for an integer
 * y in [0, 1023] the result is the correctly rounded x^y wherever that is
 * >= 2^-1000 (below: a value in [0, 2^-999]), and exactly 1.0 for y == 0
 * whatever x is (NaN included); every other y is the device library's pow
 * (pow_general), within 1e-12 relative of the exact power, with pow(0, y > 0)
 * = 0, pow(0, y < 0) = +inf and pow(1, y) = 1 exactly.  x >= 0 (shade() clamps
 * rdotv at 0).  Returns an rt_status. */
int rt_test_pow_spec(const double* x_host, const double* y_host, int n, double* out_host);

/* GPU: the specular skip of shade()'s point-light pass 2 (rt_device.hpp
 * spec_skips, RT_SPEC_SKIP) on caller-given (n, wi, wo, shininess), one lane
 * per element, launched like rt_test_pow_spec.  With rv = 2 (n.wi) n - wi as
 * shade() forms it: skip_host[i] = 1 if the trace kernels leave lane i's
 * specular term out, and plain_host[i] = pow_spec(max(0, normalized(rv) . wo),
 * shininess), what they compute where they do not.  Tests require plain_host[i]
 * to be +-0 wherever skip_host[i] is 1.  Returns an rt_status. */
int rt_test_spec_skip(const double* n_host, const double* wi_host, const double* wo_host, const double* shin_host,
                      int n, int* skip_host, double* plain_host);

/* Host only: the precomputed mt19937 tree jump polynomials in `path` (the
 * build's lib/mt19937_tree.polys, read by the jitter generator) against the
 * same polynomials computed in this process, first `levels` levels.
 * Returns 0 equal, 1 different, 2 file missing / short / corrupt. */
int rt_test_mt_poly_file(const char* path, int levels);

/* GPU, one device: the distributed frame of rt_render_dist with `world`
 * (<= 16) simulated ranks running CONCURRENTLY on the current device, one
 * host thread per rank with its own streams and device workspace, through the
 * product's rank path (dist_frame) with RCCL replaced by a same-device
 * transport that keeps its contract (host rendezvous + device copies / max
 * reduction on each rank's collective stream, timeouts): partition, row
 * chunks, both frame agreements and their verdicts, gathers, placement on the
 * root.  run->frames consecutive frames; in frame run->fault_frame rank
 * run->fault_rank gets run->fault:
 *   TRACE       its trace fails at its middle chunk (after the agreement)
 *   SETUP       it fails before its frame begins (reported in the agreement)
 *   DESC_H      it is given H + 1 (the ranks disagree on the descriptor)
 *   DESC_FLAGS  it is given flags ^ RT_FLAG_NO_CULL
 *   ABSENT      it does not take part in that frame (a dead peer; the others
 *               time out after run->timeout_ms)
 *   DESC_SCENE  it renders run->alt_scene instead (another scene content)
 *   DESC_SHED   its root strip shed (RT_ROOT_SHED_*) is one per mille higher
 * run->frame_scenes (may be NULL; entries may be NULL): frame fr renders
 * frame_scenes[fr] instead of s, on the same ranks (a rank handle reused
 * across scenes).
 * Per frame fr and rank r: run->rc[fr*world + r] (an rt_status, or
 * RT_TEST_RANK_ABSENT), run->ms[...] (the call's wall time), and the error
 * text in run->msgs[(fr*world + r) * msg_cap ...] (may be NULL).  The root's
 * frame of every successful frame fr goes to fb_host + fr*W*H*3 (doubles) or,
 * with run->rgb8, rgb8_host + fr*W*H*3 (either may be NULL).  timeout_ms <= 0:
 * RT_DIST_TIMEOUT_MS / 120 s.  Returns an rt_status for the harness itself. */
enum {
    RT_TEST_FAULT_NONE = 0,
    RT_TEST_FAULT_TRACE = 1,
    RT_TEST_FAULT_SETUP = 2,
    RT_TEST_FAULT_DESC_H = 3,
    RT_TEST_FAULT_DESC_FLAGS = 4,
    RT_TEST_FAULT_ABSENT = 5,
    RT_TEST_FAULT_DESC_SCENE = 6,
    RT_TEST_FAULT_DESC_SHED = 7
};
#define RT_TEST_RANK_ABSENT 1
typedef struct rt_test_dist_run {
    int world, rgb8, frames;
    int fault_rank, fault, fault_frame;
    int timeout_ms;
    int msg_cap;
    int* rc;
    double* ms;
    char* msgs;
    const struct rt_scene* const* frame_scenes;
    const struct rt_scene* alt_scene;
    double* split;   /* may be NULL: rt_dist_frame_split of rank r after frame fr at
                        split[(fr*world + r) * 10 ...] (successful frames) */
} rt_test_dist_run;
int rt_test_dist_threads(const struct rt_scene* s, int W, int H, int mode, int flags, rt_test_dist_run* run,
                         double* fb_host, uint8_t* rgb8_host);
/* rt_test_dist_threads for one fault-free frame: the root's frame to fb_host
 * (W*H*3 doubles) or, with rgb8, rgb8_host. */
int rt_test_render_dist_sim(const struct rt_scene* s, int W, int H, int mode, int flags, int world, int rgb8,
                            double* fb_host, uint8_t* rgb8_host);

/* GPU, one device: a world-1 rt_dist WITH a real RCCL communicator
 * (ncclCommInitRank over one rank) whose rt_render_dist frames take the
 * multi-GPU collective path (row chunks, ncclGather to root 0, placement).
 * Free with rt_dist_destroy. */
struct rt_dist;
int rt_test_dist_create_rccl1(struct rt_dist** out);
/* Fault injection on the next frame of d (rt_render_dist): 1 = this rank's
 * trace fails at its middle chunk, 2 = the collective stream is held past the
 * rank's timeout (bounded, >= 10 s: the holding kernel always ends), 3 = this
 * rank fails before its frame begins. */
int rt_test_dist_inject(struct rt_dist* d, int what);
/* CPU: Pokeball::pick_region_material's acos comparisons as thresholds
 * (rtamd::pokeball_thresholds, scene_compile.hpp): out2[0] = xb, the least x
 * in [-1, 1] with acos(x) <= btn_outer (2: none), out2[1] = xi, the greatest
 * x with acos(x) >= max(0, btn_outer - ring_width) (-2: none).  Returns 0. */
int rt_test_pokeball_thresholds(double btn_outer, double ring_width, double* out2);
/* CPU: the paper-mode output code decoder of distributed frames
 * (rtamd::paper_code_value): bits 0-2 edge index in {0, 0.3, 0.5, 0.6, 0.9},
 * bit 3 halved at the frame border, bit 4 the hatch bit (white). */
double rt_test_paper_code_value(int code);
/* CPU: the frame planners of csrc/host/frame_plan.hpp, the host-only code
 * rt_frame.hip and rt_dist.hip execute.  All return an rt_status.
 *
 * rt_test_plan_dist: rank's part of an H-row frame over `world` ranks
 * (plan_dist_frame; kind 0 = FP64 output, the root sheds strips by mode,
 * 1 = RGB8, no shed; chunks 1..4): counts[3] = {n rows, m = rows of the
 * fullest rank, n chunks}, rows_out[n], bounds_out[2 * n chunks] = (a, b) of
 * every chunk of [0, m), and with rowtab_out (cap_table >= world * m ints)
 * the root's placement table: slot world*a + r*(b-a) + (i-a) holds rank r's
 * i-th row, -1 padding. */
int rt_test_plan_dist(int H, int world, int rank, int mode, int kind, int chunks, int32_t* counts, int32_t* rows_out,
                      int32_t* bounds_out, int32_t* rowtab_out, int cap_table);
/* rt_test_plan_std: the standard-mode jitter layout of `rows` (distinct, in
 * [0, H)): jrow_out[n_rows], ranges_out[3 * n ranges] = (qa, qb, dst) of the
 * coalesced stream ranges (room for 3 * n_rows), out3 = {n ranges, q_end,
 * checkpoints needed}. */
int rt_test_plan_std(int W, int H, const int32_t* rows, int n_rows, int32_t* jrow_out, int64_t* ranges_out,
                     int64_t* out3);
/* rt_test_plan_paper: the paper-mode frame plan of `rows`: ext_out[n_ext] the
 * rows needing a primary hit and ext_shade_out[n_ext] (room for H each),
 * ext_pos_out[H], nbr_out[3 * n_rows], out6 = {n_ext, logical intersect
 * calls, ints of the aux buffer, list capacity, gtime words, waves per list
 * group}. */
int rt_test_plan_paper(int W, int H, const int32_t* rows, int n_rows, int32_t* ext_out, int32_t* ext_shade_out,
                       int32_t* ext_pos_out, int32_t* nbr_out, int64_t* out6);
/* rt_test_plan_paper_calls: that frame's trace calls calls[3k ..] = (ri0,
 * ri1, stream id), k < n_calls <= 30, through PaperCalls::next_call; after
 * call rollback_after (-1: never) rollback() is called.  call_out[4k ..] =
 * {ok, list offset, list length, bit mask of the calls it waits for}; the
 * lists back to back in lists_out (cap_lists ints); ext_done_out[n_ext] = the
 * final marks (call index + 1, 0 = not computed). */
int rt_test_plan_paper_calls(int W, int H, const int32_t* rows, int n_rows, const int32_t* calls, int n_calls,
                             int rollback_after, int32_t* call_out, int32_t* lists_out, int cap_lists,
                             int32_t* ext_done_out);
/* CPU: the paper-mode primary launch order (frame_plan.hpp order_paper_groups)
 * applied in place to list[0, n) (n a multiple of 16; entries are ext
 * indices, -1 padding), given the measured cost of the 8-entry group whose
 * first entry is e in cost[e] (0 = unmeasured).  Returns 0. */
int rt_test_paper_order(int32_t* list, int n, const uint32_t* cost, int n_cost);
/* The jitter cache of a workspace (csrc/host/jitter_cache.hpp: a standard
 * frame's draws stay resident by (W, H, rows)).  rt_test_jitter_cache_stats: of
 * the calling thread's workspace on the current device; _slot: of workspace
 * slot `slot` there (0 the process's own, r + 1 simulated rank r's, which
 * rt_test_dist_threads empties when it returns: entries and bytes are then
 * 0, the counts stay).  hits = standard frames (and jittered rt_camera_rays
 * calls, which take their draws as a frame does) that ran no jitter fill,
 * misses = those that ran it (cached or not), entries / bytes = the cached
 * buffers now (the uncached buffer is not counted).  The counts run from
 * process start or the last rt_test_jitter_cache_budget; rt_shutdown frees
 * the entries and keeps the counts.  Both take the workspace lock: not for a
 * thread between its rt_frame_begin and rt_frame_end. */
int rt_test_jitter_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* entries, uint64_t* bytes);
int rt_test_jitter_cache_stats_slot(int slot, uint64_t* hits, uint64_t* misses, uint64_t* entries, uint64_t* bytes);
/* Set the cache budget of every workspace to `bytes` (0: off; < 0: back to
 * RT_JITTER_CACHE_MB), free every cached entry and zero the counts, so that
 * one process can compare cache off, a miss and a hit.  Waits for open frames. */
int rt_test_jitter_cache_budget(int64_t bytes);
/* CPU: the cache's key / LRU / budget logic over host memory, driven by a
 * script (jitter_cache.hpp jitter_cache_sim: ops[5 * n_ops] in, out[8 * n_ops]).
 * Returns what it returns, or RT_ERR_INVALID_ARG. */
int rt_test_jitter_cache_sim(const int64_t* ops, int n_ops, int64_t budget, int64_t* out);
/* Items of one staging chunk of the batched calls' host forms (default 2^20):
 * n from here on, 0: back to the default.  It is one variable of their driver:
 * rays of rt_camera_rays (a chunk is whole rows, at least one), rays of
 * rt_query_intersect / rt_query_occluded / rt_query_radiance, hits of
 * rt_query_shade.  So that a small frame or batch crosses several chunks.
 * Process-wide; host only. */
int rt_test_camera_chunk_rays(size_t n);
/* Parents of one launch group of rt_scatter_rays_device (default and most
 * 2^30): n from here on, 0: back to the default.  So that a batch of a few
 * thousand parents crosses several groups and the child index is carried from
 * one to the next.  Process-wide; host only. */
int rt_test_scatter_launch_items(size_t n);
/* GPU: one simulated rank (rank of world) of a distributed frame on the
 * current device through the product's rank path, the RCCL gather replaced by
 * a device copy (rank 0 also places every slot).  Ranks are cached, so a
 * repeated call times a warm rank.  For per-rank timing (tools/sim_ranks.py). */
int rt_test_dist_sim_rank(const struct rt_scene* s, int W, int H, int mode, int flags, int world, int rank, int rgb8,
                          struct rt_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
