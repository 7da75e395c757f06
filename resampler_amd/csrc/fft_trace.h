// fft_trace.h -- the diagnostic builds of fft_wave.hip and fft_pair.hip (make exp EXPFILE=<file>, RSMP_EXP >> 6;
// tools/fft_trace.py): 1 = every wave's start / end on the constant 100 MHz clock and where it ran; 2 = also the
// shader-clock cycles a wave spends in each phase of its blocks (the reads of the clock drain the LDS queue at every phase
// boundary: the phases' shares are what it is for, not the total).  Included at file scope, after RSMP_EXP is defined.
#pragma once
#if (RSMP_EXP >> 6) != 0
#define RSMP_FFT_TRACE 1
__device__ unsigned long long rsmp_fft_trace_buf[4096 * 16];
extern "C" int rsmp_debug_fft_trace(unsigned long long* out, size_t words) {
    return static_cast<int>(hipMemcpyFromSymbol(out, HIP_SYMBOL(rsmp_fft_trace_buf), words * 8));
}
#endif
#if (RSMP_EXP >> 6) == 2
#define RSMP_TR(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); tr_ph[i] += t_ - tr_last; tr_last = t_; } while (0)
#else
#define RSMP_TR(i) do { } while (0)
#endif
