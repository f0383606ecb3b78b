// The one-plane and two-plane instantiations of conv_gemm_kernel ("split_planes" = 1, 2; the NP note
// in conv_gemm_kernel.h): every family that has a three-plane instantiation in conv_gemm.hip — the
// 128x128 and 64x64 forward form in its general, PW and K3 geometry, W8, and the natural-order 128x128
// weight gradient.  The Makefile compiles this file once per NP (-DMRCNN_GEMM_NP=1 / 2), beside
// conv_gemm.hip: sixteen kernels that would otherwise lengthen the longest compile of the build.
#include "conv_gemm_kernel.h"

#if !defined(MRCNN_GEMM_NP) || (MRCNN_GEMM_NP != 1 && MRCNN_GEMM_NP != 2)
#error "conv_gemm_planes.hip: compile with -DMRCNN_GEMM_NP=1 or -DMRCNN_GEMM_NP=2"
#endif

namespace mrcnn {
namespace gemm {

template <int NP>
void launch_planes(const GemmParams &p, int tile, int mode, int variant, dim3 grid, hipStream_t s, hipEvent_t ev0,
                   hipEvent_t ev1)
{
    auto go = [&](auto kernel, int threads) {
        hipExtLaunchKernelGGL(kernel, grid, dim3(threads), 0, s, ev0, ev1, 0, p);
    };
    if (tile == kW8BM) return go(conv_gemm_kernel<2, 2, FWD, false, NP, true>, 512);
    if (mode == WGRAD) return go(conv_gemm_kernel<2, 2, WGRAD, false, NP>, 256);
    auto fwd = [&](auto tm) {
        constexpr int TM = decltype(tm)::value;
        if (variant == INST_PW) return go(conv_gemm_kernel<TM, TM, FWD, false, NP, false, true>, 256);
        if (variant == INST_K3) return go(conv_gemm_kernel<TM, TM, FWD, false, NP, false, false, true>, 256);
        go(conv_gemm_kernel<TM, TM, FWD, false, NP>, 256);
    };
    if (tile == 128) fwd(std::integral_constant<int, 2>());
    else fwd(std::integral_constant<int, 1>());
}

template void launch_planes<MRCNN_GEMM_NP>(const GemmParams &, int, int, int, dim3, hipStream_t, hipEvent_t,
                                           hipEvent_t);

}  // namespace gemm
}  // namespace mrcnn
