// Stand-in for <hip/hip_runtime.h> when a host/device header of csrc/ (fvm_row.hpp, row_index3.hpp) is compiled by the host
// compiler alone for a CPU test: the function qualifiers mean nothing there.
#pragma once
#define __host__
#define __device__
