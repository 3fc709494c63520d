// Resident workgroups per CU of the attention forward kernels, from the HIP occupancy API
// (build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include tools/occupancy.hip -o /tmp/occ)
#include "../knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd/csrc/attention.hip"
#include <cstdio>

namespace kd { int fail(int code, const std::string&) { return code; } }

template <typename K> static void show(const char* name, K k, size_t smem) {
    int n = -1;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 256, smem);
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, (const void*)k);
    printf("%-40s smem %6zu  blocks/CU %d (%s)  regs %d  static lds %zu\n", name, smem, n, hipGetErrorString(e), a.numRegs,
           a.sharedSizeBytes);
}

int main() {
    using namespace kd;
    show("k_attn_fwd<128,true,2>", k_attn_fwd<128, true, 2>, 65536);
    show("fwd32<128,true,F32_DMA>", fwd32<128, true, F32_DMA>(), 65536);
    show("fwd32<128,false,F32_DMA>", fwd32<128, false, F32_DMA>(), 65536);
    show("fwd32<128,true,F32_REGSTAGE>", fwd32<128, true, F32_REGSTAGE>(), 65536);
    show("fwd32<64,true,F32_DMA>", fwd32<64, true, F32_DMA>(), 32768);
    show("fwd32<96,false,F32_DMA>", fwd32<96, false, F32_DMA>(), 65536);
    show("fwd32<128,true,F32_DMA> 48K", fwd32<128, true, F32_DMA>(), 49152);
    int dev = 0; hipDeviceProp_t pr{};
    (void)hipGetDeviceProperties(&pr, dev);
    printf("sharedMemPerMultiprocessor %zu maxSharedMemoryPerMultiProcessor %zu sharedMemPerBlock %zu\n",
           pr.sharedMemPerBlock, pr.maxSharedMemoryPerMultiProcessor, pr.sharedMemPerBlock);
    return 0;
}
