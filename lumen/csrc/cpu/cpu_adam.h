// Host AdamW entry points (cpu_adam.cpp), declared once for their definition, binding.cpp and the
// sanitizer harness.  Separate from kernels/api.h: cpu_adam.cpp is compiled without the ROCm
// include path.
#pragma once

extern "C" {
int lumen_cpu_has_avx512();
void lumen_cpu_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float b1,
                     float b2, float eps, float wd, float bc1, float bc2, float grad_scale);
}
