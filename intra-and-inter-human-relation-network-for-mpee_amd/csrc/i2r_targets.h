// The definition of a (crop, joint) target map, shared by the kernels that evaluate it in place (i2r_metrics.hip: i2r_joint_targets,
// i2r_val_metrics; i2r_head_fit.hip: i2r_head_grad): generate_target + adjust_target_weight of lib/dataset/JointsDataset.py:394-450.
#pragma once
#include "i2r_common.h"

// Every product and difference of the reference is a rounding of its own (numpy's float64 steps of the Gaussian's argument, torch's fp32
// operations of a loss term).  HIP device code contracts a * b - c to an FMA by default, so contraction is switched off here and stays
// off for the rest of the including file (i2r_metrics.hip says why __fmul_rn / __fsub_rn do not do it).
#pragma clang fp contract(off)

// adjust_target_weight (JointsDataset.py:438-450) + the draw decision of generate_target (:418, :429) + joints_weight (:432-433).
// int() truncates toward zero; the comparisons are made on the truncated doubles, so a far-away mu cannot overflow an int.
__device__ inline float joint_weight(double mx, double my, float vis, const float* jw, int j, double sigma, int h, int w, bool* draw) {
    const double tmp = sigma * 3.0;
    float tw = vis;
    if (trunc(mx - tmp) >= (double)w || trunc(my - tmp) >= (double)h || trunc(mx + tmp + 1.0) < 0.0 || trunc(my + tmp + 1.0) < 0.0) tw = 0.f;
    *draw = tw > 0.5f;  // (a weight in (0, 0.5] leaves the map zero but still reaches the loss)
    return jw ? tw * jw[j] : tw;
}

// np.exp(-((x - mu_x) ** 2 + (y - mu_y) ** 2) / (2 * sigma ** 2)) of float32 pixel coordinates and a float64 mu: the argument in fp64
// as the reference has it, rounded to fp32, one expf (the reference rounds a float64 exp once: within 4 fp32 ulp of it)
__device__ inline float gauss(int x, int y, double mx, double my, double two_s2) {
    const double dx = (double)x - mx, dy = (double)y - my;
    return expf((float)(-(dx * dx + dy * dy) / two_s2));
}
