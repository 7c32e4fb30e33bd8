// rt_kernel_table.hpp — the one form of the kernel tables, built per namespace
// right after rt_device.hpp, ahead of the kernels of rt_kernels.hpp,
// rt_query_kernels.hpp, rt_radiance_kernels.hpp or rt_shade_kernels.hpp (a
// translation unit includes one of them).  Host code only.
//
// A table is an array of rows, one kernel each, written with RT_KERNEL_ROW so
// that a row's name is its instantiation as spelled there: the name rocprofv3
// prints.  A row answers to a key its table packs from the KernelVariant
// fields it has columns for; a variant without a row has no kernel in this
// namespace, and its launch is an error, never another kernel.  What the host
// sees of a table is a rtamd::KernelTable (rt_launch.hpp).

namespace RT_NS {
namespace {

template <class... A>
struct KernelRow {
    unsigned key;
    void (*fn)(A...);
    const char* name;
};
#define RT_KERNEL_ROW(key, ...) {key, __VA_ARGS__, #__VA_ARGS__}

template <class R, size_t N>
const R* find_kernel(const R (&table)[N], unsigned key) {
    for (const R& r : table)
        if (r.key == key) return &r;
    return nullptr;
}
// Row i of a table as written (nullptr past the end)
template <class R, size_t N>
const char* row_name(const R (&table)[N], int i) {
    return i >= 0 && i < (int)N ? table[i].name : nullptr;
}
// A row's kernel and name (resource queries); {nullptr, nullptr}: no row
template <class R>
rtamd::KernelEntry kernel_entry(const R* k) {
    return k ? rtamd::KernelEntry{(const void*)k->fn, k->name} : rtamd::KernelEntry{nullptr, nullptr};
}

// The batched kernels' launch: item i of p's batch of p.n is lane i % 64 of the
// one-wave workgroup i / 64, one launch over the whole batch (p.n > 0, at most
// 2^31 - 1 waves: the host splits larger batches).  pool: the dynamic LDS.
// own_lights: V.lights / V.n_lights are the call's point lights, not the
// scene's, so the kernel gets no light-relative cull records (indexed by the
// scene's own light numbers: WV kernels only).
constexpr int kQueryThreads = 64;
template <class P>
hipError_t launch_lanes(const KernelRow<DevScene, P>* k, size_t pool, bool own_lights, hipStream_t st,
                        const rtamd::SceneView& V, const P& p) {
    if (!k) return hipErrorInvalidDeviceFunction;
    const size_t waves = (p.n + kQueryThreads - 1) / kQueryThreads;
    if (!p.n || waves > 0x7fffffffu) return hipErrorInvalidValue;
    DevScene S = make_scene(V);
    if (own_lights) S.lrec = S.lgb = nullptr;
    rtamd::note_launch(kNsName, k->name);
    hipLaunchKernelGGL(k->fn, dim3((unsigned)waves), dim3(kQueryThreads), pool, st, S, p);
    return hipGetLastError();
}

}  // namespace
}  // namespace RT_NS
