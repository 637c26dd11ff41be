// ubench_fetch.hip -- calibration of rocprofv3's FETCH_SIZE on KNOWN byte counts, for the access patterns of the TSDF update kernel
// (the MI355X guide: FETCH_SIZE reports half the bytes of 16-B-per-lane streaming reads on gfx950; other widths must be calibrated).
//   read8:   every lane reads 8 B, a wave 512 contiguous bytes (the record runs of a sub-brick), N bytes in all, read once
//   read16:  every lane reads 16 B (the guide's case)
//   gather4: every lane reads 4 B at a pseudo-random pixel of a 265 MB pool of 32 images (the depth gathers; N lane-reads)
// Build + run under the profiler on the GPU box:
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_fetch.hip -o /tmp/ubench_fetch
//   rocprofv3 --pmc FETCH_SIZE --output-format csv -d out -- /tmp/ubench_fetch
// and compare FETCH_SIZE (KB) x 1024 of each kernel with the bytes it prints.
#include <hip/hip_runtime.h>
#include <stdio.h>

__global__ void read8(const int2 *p, size_t n, int *sink) {
    int acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { const int2 v = p[i]; acc += v.x ^ v.y; }
    if (acc == 0x7fffffff) *sink = acc;
}
__global__ void read16(const int4 *p, size_t n, int *sink) {
    int acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { const int4 v = p[i]; acc += v.x ^ v.y ^ v.z ^ v.w; }
    if (acc == 0x7fffffff) *sink = acc;
}
__global__ void gather4(const float *p, size_t npix, size_t reads_per_thread, int *sink) {
    float acc = 0.f;
    unsigned long long s = (unsigned long long)(blockIdx.x * blockDim.x + threadIdx.x) * 0x9E3779B97F4A7C15ull + 12345ull;
    for (size_t k = 0; k < reads_per_thread; ++k) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        acc += p[(size_t)(s >> 20) % npix];
    }
    if (acc == 1.2345f) *sink = 1;
}

int main() {
    const size_t bytes = (size_t)1 << 30;            // 1 GiB streamed once by read8 / read16 (past the 256 MiB Infinity Cache)
    const size_t pool = (size_t)32 * 1080 * 1920;    // pixels of 32 depth images (265 MB)
    void *buf = nullptr; int *sink = nullptr;
    if (hipMalloc(&buf, bytes) != hipSuccess || hipMalloc(&sink, 4) != hipSuccess) return 1;
    (void)hipMemset(buf, 1, bytes);
    (void)hipDeviceSynchronize();
    hipLaunchKernelGGL(read8, dim3(4096), dim3(256), 0, 0, (const int2 *)buf, bytes / 8, sink);
    hipLaunchKernelGGL(read16, dim3(4096), dim3(256), 0, 0, (const int4 *)buf, bytes / 16, sink);
    const size_t rpt = 64;
    hipLaunchKernelGGL(gather4, dim3(4096), dim3(256), 0, 0, (const float *)buf, pool, rpt, sink);
    (void)hipDeviceSynchronize();
    printf("read8 bytes %zu\nread16 bytes %zu\ngather4 lane_reads %zu (x 4 B = %zu useful bytes; x 64 B lines = %zu)\n", bytes, bytes,
           (size_t)4096 * 256 * rpt, (size_t)4096 * 256 * rpt * 4, (size_t)4096 * 256 * rpt * 64);
    return 0;
}
