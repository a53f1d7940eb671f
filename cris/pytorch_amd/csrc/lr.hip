// Per-step learning-rate schedule inside the training step (NativeTrainer(lr_schedule=...), ops.LrSchedule):
//   cris_adam_schedule_lrs   one launch per Adam table: the `lr` field of every descriptor <- lr_table[row of this step][its group]
// The row is chosen on the device from the optimizer step counter, so a captured graph or a recorded command list replays the
// launch unchanged; the Adam kernels that follow read `lr` from the same table at every launch.  Values are copied, never
// computed: whatever schedule filled the table on the host is followed bit for bit.
#include "common.h"
#include "../../../include/cris_hip.h"

// Thread i owns descriptor i and stores one float into it; nothing else of the 112 bytes is written.  A group index outside the
// table (the host refuses it: ops.LrSchedule) leaves the descriptor alone rather than reading past the row.
__global__ __launch_bounds__(256) void adam_schedule_lrs_kernel(cris_adam_desc* tab, int n_desc, const uint8_t* __restrict__ group_of,
                                                                const int* __restrict__ step, const float* __restrict__ lr_table,
                                                                int n_rows, int n_groups, float* lr_out) {
    const int s = step[0];                       // 1-based optimizer step (cris_step_advance[_micro] ran before)
    int row = s - 1;
    row = row < 0 ? 0 : row;
    row = row > n_rows - 1 ? n_rows - 1 : row;   // steps past the end keep the last row
    const float* __restrict__ rates = lr_table + (long)row * n_groups;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_desc) {
        const int g = group_of[i];
        if (g < n_groups) tab[i].lr = rates[g];
    }
    if (lr_out && blockIdx.x == 0 && (int)threadIdx.x < n_groups) lr_out[threadIdx.x] = rates[threadIdx.x];      // (n_groups <= 255)
}

extern "C" int cris_adam_schedule_lrs(cris_adam_desc* dev_table, int n_desc, const uint8_t* group_of, const int32_t* step_dev,
                                      const float* lr_table, int n_rows, int n_groups, float* lr_out, void* stream) {
    CRIS_CHECK_ARG(dev_table && group_of && step_dev && lr_table, "null table, group_of, step counter or lr_table");
    CRIS_CHECK_ARG(n_desc >= 1, "n_desc must be >= 1");
    CRIS_CHECK_ARG(n_rows >= 1, "n_rows must be >= 1");
    CRIS_CHECK_ARG(n_groups >= 1 && n_groups <= 255, "n_groups must lie in [1, 255]");
    hipLaunchKernelGGL(adam_schedule_lrs_kernel, dim3(cris_cdiv(n_desc, 256)), dim3(256), 0, (hipStream_t)stream, dev_table, n_desc,
                       group_of, step_dev, lr_table, n_rows, n_groups, lr_out);
    CRIS_LAUNCH_CHECK();
    return 0;
}
