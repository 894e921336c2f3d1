// scenario_layout.h — the flat scenario-major layout of ign_forward_scenarios, for the
// kernels (scenario.hip) and the host driver (scenario.cpp) alike.  No HIP header.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define IGN_SCEN_HD __host__ __device__
#else
#define IGN_SCEN_HD
#endif

// Sp: the scenarios rounded up to whole 16-row tiles
IGN_SCEN_HD inline int64_t scen_padded(int64_t n_scen) { return (n_scen + 15) / 16 * 16; }
// first float of scenario s of row `row` in an array [rows][sp][width]
IGN_SCEN_HD inline int64_t scen_offset(int64_t row, int64_t s, int64_t sp, int width) { return (row * sp + s) * width; }
// floats of such an array
IGN_SCEN_HD inline int64_t scen_floats(int64_t rows, int64_t sp, int width) { return rows * sp * width; }
