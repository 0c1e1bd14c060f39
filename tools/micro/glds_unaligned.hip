// Development check for gfx950: two facts about global_load_lds_dword that k_fast_cells' LDS-DMA staging would rely on.
//  1. A lane whose global address sits 1, 2 or 3 bytes past a dword boundary (level-0 cells read from a caller's image with
//     an odd row stride) must deliver the same four bytes as an ordinary unaligned global_load_dword + ds_write_b32.
//  2. A lane that is masked off (EXEC = 0) must leave its LDS dword (M0 base + 4 * lane) untouched.
// One launch, a few one-wavefront workgroups.  Every workgroup stages kGroups row groups of kRows rows x kSW dwords
// (lane = row * kSW + column, 55 live lanes) from a byte-patterned buffer both ways, at source byte offsets 0..3, and
// counts differing dwords and overwritten sentinel dwords.  All addresses stay inside the program's own allocations:
// the highest source byte read is 3 + (kGroups * kRows - 1) * kPitch + 4 * kSW - 1 < kBytes, the LDS image is
// kGroups * 64 dwords per copy.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>

constexpr int kSW = 11, kRows = 64 / kSW, kLive = kRows * kSW, kGroups = 8, kPitch = 1241, kBytes = 64 * 1024;
static_assert(3 + (kGroups * kRows - 1) * kPitch + 4 * kSW <= kBytes, "source reads stay inside the buffer");

__global__ __launch_bounds__(64) void k_glds(const uint8_t *__restrict__ src, unsigned long long *bad)
{
    __shared__ uint32_t ref[kGroups * 64], dma[kGroups * 64];
    const int lane = threadIdx.x, r = lane / kSW, c = lane - r * kSW;
    const uint32_t sentinel = 0xa5000000u | (blockIdx.x << 8) | lane;
    for (int a = 0; a < 4; ++a) {
        const uint8_t *sb = src + a + (blockIdx.x & 7) * 4;
        for (int g = 0; g < kGroups; ++g) { ref[g * 64 + lane] = sentinel; dma[g * 64 + lane] = sentinel; }
        __syncthreads();
        if (lane < kLive) {
            const uint32_t voff = (uint32_t)(r * kPitch + 4 * c);
            for (int g = 0; g < kGroups; ++g) {
                // the statement k_fast_cells issues: scalar row base + the lane's 32-bit offset, LDS base in M0
                const uintptr_t rowp = reinterpret_cast<uintptr_t>(sb) + (uint32_t)(g * kRows * kPitch);
                const uint32_t dst = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint32_t *)(dma + g * 64));
                uint32_t keep;
                ref[g * 64 + lane] = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(rowp) + voff);
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(voff), "s"(rowp), "s"(dst) : "memory");
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        unsigned diff = 0, touched = 0;
        for (int g = 0; g < kGroups; ++g) {
            const uint32_t x = ref[g * 64 + lane], y = dma[g * 64 + lane];
            if (lane < kLive) diff += x != y;
            else touched += y != sentinel;
        }
        if (diff) atomicAdd(&bad[a], (unsigned long long)diff);
        if (touched) atomicAdd(&bad[4], (unsigned long long)touched);
        __syncthreads();
    }
}

int main()
{
    std::vector<uint8_t> h(kBytes);
    uint32_t s = 12345u;
    for (int i = 0; i < kBytes; ++i) { s = s * 1664525u + 1013904223u; h[i] = (uint8_t)(s >> 24); }
    uint8_t *d_src;
    unsigned long long *d_bad, hb[5] = {0, 0, 0, 0, 0};
    if (hipMalloc(&d_src, kBytes) != hipSuccess || hipMalloc(&d_bad, sizeof(hb)) != hipSuccess) { printf("no device memory\n"); return 2; }
    (void)hipMemcpy(d_src, h.data(), kBytes, hipMemcpyHostToDevice);
    (void)hipMemset(d_bad, 0, sizeof(hb));
    hipLaunchKernelGGL(k_glds, dim3(64), dim3(64), 0, 0, d_src, d_bad);
    const hipError_t err = hipDeviceSynchronize();
    (void)hipMemcpy(hb, d_bad, sizeof(hb), hipMemcpyDeviceToHost);
    printf("64 workgroups x %d groups x %d live lanes: differing dwords at source byte offset 0/1/2/3: %llu/%llu/%llu/%llu, "
           "masked-off lanes' LDS dwords overwritten: %llu, last error: %s\n",
           kGroups, kLive, hb[0], hb[1], hb[2], hb[3], hb[4], hipGetErrorString(err));
    return err != hipSuccess || hb[0] || hb[1] || hb[2] || hb[3] || hb[4];
}
