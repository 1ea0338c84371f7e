// Cycles per v_mfma_f64_16x16x4_f64 (the shared block search's instruction, csrc/vec_kernels_shared.h): the guides give no
// issue rate for it on gfx950.  N MFMAs back to back per wave, one workgroup per CU; 1 wave per SIMD with ACC = 1 (each
// MFMA waits for the one before: the dependent latency) and ACC = 2 / 4 independent accumulators (the issue interval), and 2
// waves per SIMD.  Cycles = the event time at the clock the device reports; the achieved chip rate in TFLOP/s needs no clock.
//   hipcc --offload-arch=gfx950 -O3 tools/mfma_f64_rate.hip -o /tmp/mfma_f64_rate
#include <hip/hip_runtime.h>
#include <cstdio>

typedef double __attribute__((ext_vector_type(4))) d4;

template <int ACC>
__global__ void rate_kernel(double *out, int iters, double seed) {
    d4 acc[ACC];
#pragma unroll
    for (int i = 0; i < ACC; ++i) acc[i] = d4{seed, 0.0, 0.0, 0.0};
    const double a = seed + 1e-3 * (double)threadIdx.x, b = seed - 1e-3 * (double)threadIdx.x;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 8 / ACC; ++u)
#pragma unroll
            for (int i = 0; i < ACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < ACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) out[0] = s;
}

template <int ACC>
static void run(int waves_per_cu, int cus, double mhz) {
    double *out;
    (void)hipMalloc(&out, 64);
    const int iters = 20000;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    rate_kernel<ACC><<<cus, 64 * waves_per_cu>>>(out, 1000, 0.5);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    rate_kernel<ACC><<<cus, 64 * waves_per_cu>>>(out, iters, 0.5);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double n = (double)iters * 8;  // MFMAs per wave
    const double ns = ms * 1e6 / n, waves_per_simd = waves_per_cu / 4.0;
    const double cyc = ns * mhz * 1e-3 / waves_per_simd;  // cycles per MFMA and SIMD at the reported clock
    const double tflops = 2.0 * 16 * 16 * 4 * n * waves_per_cu * cus / (ms * 1e-3) * 1e-12;
    printf("| %d | %d | %.3f | %.2f | %.1f | %.1f |\n", ACC, waves_per_cu / 4, ms, ns, cyc, tflops);
    (void)hipFree(out);
}

int main() {
    hipDeviceProp_t p;
    (void)hipGetDeviceProperties(&p, 0);
    const int cus = p.multiProcessorCount;
    const double mhz = p.clockRate * 1e-3;
    printf("%s, %d CUs, reported clock %.0f MHz; 20000 x 8 v_mfma_f64_16x16x4_f64 per wave, one workgroup per CU\n\n", p.name, cus, mhz);
    printf("| independent accumulators | waves per SIMD | ms | ns per MFMA and wave | cycles per MFMA and SIMD at the reported clock | chip TFLOP/s (f64) |\n");
    printf("|---|---|---|---|---|---|\n");
    run<1>(4, cus, mhz);
    run<2>(4, cus, mhz);
    run<4>(4, cus, mhz);
    run<1>(8, cus, mhz);
    run<4>(8, cus, mhz);
    return 0;
}
