/* sim3opt_bench.h -- measurement hooks of libsim3opt: NOT part of the drop-in interface
 * (include/sim3opt.h is what a maintainer of the reference binds).  bench.py and the tuning scripts
 * under scripts/ use them to time single kernels on a graph that is already resident in HBM. */
#ifndef SIM3OPT_BENCH_H
#define SIM3OPT_BENCH_H

#include "sim3opt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* times `reps` back-to-back launches of the block-CSR SpMV kernel; returns mean ms */
int sim3opt_bench_spmv(sim3opt_graph* g, int32_t reps, double* ms_mean);
/* HBM read calibration over the same value array (bench only): mode 0 = 16 B/lane contiguous,
 * 1 = 8 B/lane contiguous, 2 = 8 B/lane on 49 of 64 lanes per 392-B block (the SpMV's shape) */
int sim3opt_bench_stream(sim3opt_graph* g, int32_t mode, int32_t reps, double* ms_mean);

#ifdef __cplusplus
}
#endif

#endif /* SIM3OPT_BENCH_H */
