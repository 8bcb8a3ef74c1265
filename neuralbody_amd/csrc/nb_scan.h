// Internal: device-wide exclusive scan (nb_scan.hip).
#pragma once
#include "nb_common.h"

long long nb_scan_blocks(long long n);
// out[i] = sum_{k<i} flags[k]; *total = sum of all flags.  block_sums: nb_scan_blocks(n) ints.
int nb_exclusive_scan(const int *flags, int *out, int *total, long long n, int *block_sums, hipStream_t st);
// exclusive scan of n_blocks block sums in place (one block; the step between count and place beyond nbscan::FUSED_MAX_BLOCKS).
// Launches without a check of its own: the caller's NB_CHECK_LAUNCH behind the place launch covers it.
void nb_scan_tops(int *block_sums, int n_blocks, hipStream_t st);
// split a scratch buffer of nb_scan_scratch_size(n) bytes into [flags n][pos n][block sums]; a NULL argument: that section is not used
void nb_scan_carve(void *scratch, long long n, int **flags, int **pos, int **block_sums);
// the spare int behind the carve's block sums, for a total that stays on the device (see nb_scan_scratch_size)
static inline int *nb_scan_total_slot(int *block_sums, long long n) { return block_sums + nb_scan_blocks(n); }
