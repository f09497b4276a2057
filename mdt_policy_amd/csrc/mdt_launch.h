// mdt_launch.h -- host-side launch plumbing of the kernel sources: the per-device lookup, the one place that raises a kernel's
// dynamic-LDS limit, and the runtime-value -> template-constant dispatch the launchers share.  Everything here has internal
// linkage: nothing of it shows among the library's dynamic symbols.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

constexpr int MDT_MAX_DEVICES = 32;
// the current device's slot in a per-device table (slot 0 when the index cannot be had or is out of range)
static inline int mdt_current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MDT_MAX_DEVICES) return 0;
    return dev;
}

// Launch Kernel with `lds` bytes of dynamic LDS.  hipFuncAttributeMaxDynamicSharedMemorySize is kept at the largest size this
// instantiation has asked for on the current device (function attributes are per device) and raised only when a launch asks
// for more, so a launcher's size may depend on the shape and a steady state makes no host call beside the launch.
template <auto Kernel, class... Args>
static hipError_t mdt_launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
    static size_t mark_dev[MDT_MAX_DEVICES] = {0};
    size_t& mark = mark_dev[mdt_current_device()];
    if (lds > mark) {
        hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        mark = lds;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
    return hipGetLastError();
}

// f(std::integral_constant<int, v>()) for Lo <= v <= Hi -- f is a generic lambda that uses decltype(c)::value as a template
// argument, so exactly the instantiations Lo..Hi exist; any other v is refused (a caller that clamps does so in the argument).
template <int Lo, int Hi, class F>
static hipError_t mdt_with_const(int v, F f) {
    if (v == Lo) return f(std::integral_constant<int, Lo>());
    if constexpr (Lo < Hi) return mdt_with_const<Lo + 1, Hi>(v, f);
    else return hipErrorInvalidValue;
}
