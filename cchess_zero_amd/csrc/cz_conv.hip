// cz_conv.hip — the C-ABI entry points of the MFMA conv kernels (device code: cz_conv_kernel.h, cz_trunk_split.h, cz_trunk_mx.h).
// The six one-launch trunk entries are a TrunkEntry each and one call of launch_trunk.  The variants that were measured and not
// adopted are not launched from here: tools/experiments/patches/mx_variants_hook.patch adds their hook to the
// copy of the sources that tools/experiments/mx_ablate.sh builds.
#include "cz_internal.h"
#include "cz_conv_kernel.h"
#include "cz_trunk_split.h"
#include "cz_trunk_mx.h"
#include <initializer_list>
#include <type_traits>

#define CZ_KERNEL(...) reinterpret_cast<const void *>(__VA_ARGS__)

// the dynamic-LDS opt-in of a kernel family (both dtypes together; NULL: no second kernel), on its first launch in this context
static int lds_opt_in(cz_ctx *c, int family, int lds_bytes, const void *k0, const void *k1 = nullptr) {
    if (c->lds_opt_in[family]) return CZ_OK;
    for (const void *k : {k0, k1})
        if (k) CZ_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    c->lds_opt_in[family] = true;
    return CZ_OK;
}

extern "C" int cz_conv3x3_c128_bf16(cz_ctx *c, const void *in, const void *wpk, const float *bias, const void *residual,
                                    void *out, int B, int relu) {
    using namespace czconv;
    CZ_REQUIRE(c && in && wpk && bias && out && B >= 0, "cz_conv3x3_c128_bf16: null argument");
    if (B == 0) return CZ_OK;
    if (const int rc = lds_opt_in(c, CZ_LDS_CONV, CV_LDS_BYTES, CZ_KERNEL(k_conv3x3_c128))) return rc;
    const int grid = (B + CV_P - 1) / CV_P;
    hipLaunchKernelGGL(k_conv3x3_c128, dim3(grid), dim3(CV_THREADS), CV_LDS_BYTES, c->stream, (const uint16_t *)in,
                       (const uint16_t *)wpk, bias, (const uint16_t *)residual, (uint16_t *)out, B, relu);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

// cz_set_clock_probe: the trunk kernels stamp every workgroup's start / end in both clocks when the buffer holds the grid
static unsigned long long *clock_probe(cz_ctx *c, int grid) {
    if (!c->clock_probe || grid > c->clock_probe_wgs) return nullptr;
    c->clock_probe_last_grid = grid;
    return c->clock_probe;
}

// In front of every one-launch trunk kernel's launch: the alignment checks (wpk16: the weights where the kernel fetches them by
// 16-byte DMA from their first byte, else NULL) and the grid at P positions per workgroup.  `who` names the entry point in
// errors.  *grid == 0 on success: B == 0, nothing to launch.
static int trunk_grid(const char *who, const float *head_w, const void *wpk16, int B, int P, int *grid) {
    *grid = 0;
    if (head_w && (reinterpret_cast<uintptr_t>(head_w) & 15u)) { cz_set_error("%s: head_w must be 16-byte aligned", who); return CZ_EINVAL; }
    if (reinterpret_cast<uintptr_t>(wpk16) & 15u) { cz_set_error("%s: wpk must be 16-byte aligned", who); return CZ_EINVAL; }
    *grid = (B + P - 1) / P;
    return CZ_OK;
}

// What differs between the one-launch trunk entry points.  K: the kernels' type — their leading parameters, then
// (B, layers, the device row count, the clock probe)
template <typename K>
struct TrunkEntry {
    const char *name;         // in the argument errors
    const char *align_name;   // in the alignment errors
    K kernel[2];              // what `which` chooses between (one kernel: the second is NULL); opted in together
    int lds_bytes, threads, P, family;   // dynamic LDS, workgroup size, positions per workgroup, the CzLdsFamily of the opt-in
    bool wpk16;               // the weights are fetched by 16-byte DMA from their first byte
};

// One trunk launch, whole: the argument checks in their order, the grid (B == 0: CZ_OK, nothing is launched or opted in), the
// opt-in, the launch of kernel[which] with (lead..., B, 2 * nblocks, row count, clock probe).  given: the entry's own pointers
// and counts are there; which < 0: cz_net_trunk_split's halves_dtype names neither kernel.
template <typename K, typename... L>
static int launch_trunk(cz_ctx *c, const TrunkEntry<K> &e, int which, bool given, const void *wpk, const float *head_w, const float *head_b,
                        const float *head_out, int B, int nblocks, L... lead) {
    static_assert(std::is_same_v<K, void (*)(L..., int, int, const int32_t *, unsigned long long *)>, "the launch arguments are the kernel's parameters, type by type");
    if (!given) { cz_set_error("%s: null argument / nblocks < 1", e.name); return CZ_EINVAL; }
    if (head_out && !(head_w && head_b)) { cz_set_error("%s: head_out needs head_w and head_b", e.name); return CZ_EINVAL; }
    if (which < 0) { cz_set_error("%s: halves_dtype must be CZ_F16 or CZ_BF16", e.name); return CZ_EINVAL; }
    int grid;
    if (const int rc = trunk_grid(e.align_name, head_w, e.wpk16 ? wpk : nullptr, B, e.P, &grid); rc != CZ_OK || grid == 0) return rc;
    if (const int rc = lds_opt_in(c, e.family, e.lds_bytes, CZ_KERNEL(e.kernel[0]), CZ_KERNEL(e.kernel[1]))) return rc;
    hipLaunchKernelGGL(e.kernel[which], dim3(grid), dim3(e.threads), e.lds_bytes, c->stream, lead..., B, 2 * nblocks, c->batch_count,
                       clock_probe(c, grid));
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

// the three entry points of k_tower8_c128 (their alignment errors share one name); f16: the fp16 instantiation
static int launch_tower(cz_ctx *c, const char *name, bool given, bool f16, const void *in, const void *wpk, const float *bias, void *out,
                        const float *head_w, const float *head_b, float *head_out, int B, int nblocks, const void *planes = nullptr,
                        const void *w0 = nullptr, const float *b0 = nullptr) {
    using namespace czconv;
    const TrunkEntry<decltype(&k_tower8_c128<false, 4>)> e = {name, "cz_net_trunk", {k_tower8_c128<false, 4>, k_tower8_c128<true, 4>},
                                                              T8_LDS_BYTES, T8_THREADS, T8_P, CZ_LDS_TOWER, false};
    return launch_trunk(c, e, f16 ? 1 : 0, given, wpk, head_w, head_b, head_out, B, nblocks, (const uint16_t *)in, (const uint16_t *)wpk, bias,
                        (uint16_t *)out, head_w, head_b, head_out, (const uint16_t *)planes, (const uint16_t *)w0, b0);
}

extern "C" int cz_tower_c128_bf16(cz_ctx *c, const void *in, const void *wpk, const float *bias, void *out, int B, int nblocks) {
    return launch_tower(c, "cz_tower_c128_bf16", c && in && wpk && bias && out && B >= 0 && nblocks >= 1, false, in, wpk, bias, out, nullptr,
                        nullptr, nullptr, B, nblocks);
}

extern "C" int cz_tower_heads_c128_bf16(cz_ctx *c, const void *in, const void *wpk, const float *bias, void *trunk_out,
                                        const float *head_w, const float *head_b, float *head_out, int B, int nblocks) {
    return launch_tower(c, "cz_tower_heads_c128_bf16", c && in && wpk && bias && head_w && head_b && head_out && B >= 0 && nblocks >= 1, false,
                        in, wpk, bias, trunk_out, head_w, head_b, head_out, B, nblocks);
}

// what the four whole-net entry points ask of their arguments, under the names all four give them
#define CZ_NET_GIVEN (c && planes16 && w0 && b0 && wpk && bias && B >= 0 && nblocks >= 1 && (trunk_out || head_out))

extern "C" int cz_net_trunk_bf16(cz_ctx *c, const void *planes16, const void *w0, const float *b0, const void *wpk,
                                 const float *bias, void *trunk_out, const float *head_w, const float *head_b,
                                 float *head_out, int B, int nblocks) {
    return launch_tower(c, "cz_net_trunk_bf16", CZ_NET_GIVEN, false, nullptr, wpk, bias, trunk_out, head_w, head_b, head_out, B, nblocks, planes16, w0, b0);
}

extern "C" int cz_net_trunk_f16(cz_ctx *c, const void *planes16, const void *w0, const float *b0, const void *wpk,
                                const float *bias, void *trunk_out, const float *head_w, const float *head_b,
                                float *head_out, int B, int nblocks) {
    return launch_tower(c, "cz_net_trunk_f16", CZ_NET_GIVEN, true, nullptr, wpk, bias, trunk_out, head_w, head_b, head_out, B, nblocks, planes16, w0, b0);
}

extern "C" int cz_net_trunk_split(cz_ctx *c, const void *planes16, const void *w0, const float *b0, const void *wpk,
                                  const float *bias, float *trunk_out, const float *head_w, const float *head_b,
                                  float *head_out, int B, int nblocks, int halves_dtype) {
    using namespace czconv;
    static const TrunkEntry<decltype(&k_trunk_split_c128<false>)> e = {"cz_net_trunk_split", "cz_net_trunk_split", {k_trunk_split_c128<false>, k_trunk_split_c128<true>},
                                                                       XS_LDS_BYTES, XS_THREADS, XS_P, CZ_LDS_SPLIT, false};
    return launch_trunk(c, e, halves_dtype == CZ_F16 ? 1 : halves_dtype == CZ_BF16 ? 0 : -1, CZ_NET_GIVEN, wpk, head_w, head_b, head_out, B, nblocks,
                        (const uint16_t *)wpk, bias, trunk_out, head_w, head_b, head_out, (const uint16_t *)planes16, (const uint16_t *)w0, b0);
}

extern "C" int cz_net_trunk_mx(cz_ctx *c, const void *planes16, const void *w0, const float *b0, const void *wpk, const float *bias,
                               float *trunk_out, const float *head_w, const float *head_b, float *head_out, int B, int nblocks) {
    using namespace czconv;
    static const TrunkEntry<decltype(&k_trunk_mx_c128)> e = {"cz_net_trunk_mx", "cz_net_trunk_mx", {k_trunk_mx_c128, nullptr}, MX_LDS_BYTES, MX_THREADS, MX_P, CZ_LDS_MX, true};
    return launch_trunk(c, e, 0, CZ_NET_GIVEN, wpk, head_w, head_b, head_out, B, nblocks, (const unsigned char *)wpk, bias, trunk_out, head_w,
                        head_b, head_out, (const uint16_t *)planes16, (const uint16_t *)w0, b0);
}

extern "C" int cz_set_clock_probe(cz_ctx *c, unsigned long long *buf_dev, int max_workgroups) {
    CZ_REQUIRE(c && max_workgroups >= 0, "cz_set_clock_probe: null context");
    c->clock_probe = buf_dev;
    c->clock_probe_wgs = buf_dev ? max_workgroups : 0;
    c->clock_probe_last_grid = 0;
    return CZ_OK;
}

extern "C" int cz_clock_probe_last_grid(cz_ctx *c) { return c ? c->clock_probe_last_grid : 0; }
