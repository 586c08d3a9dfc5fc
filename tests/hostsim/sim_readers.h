// How the CPU simulations of the row and padded passes (rows_sim.cpp, padded_sim.cpp) hand the caller's arrays to the functions they
// share with the kernels: every index is checked, and one out of bounds sets *oob instead of being read.
#pragma once
#include <stdint.h>

struct SimOffsets {
    const uint64_t* p;
    uint64_t n_docs;
    bool* oob;
    uint64_t operator[](uint64_t d) const {
        if (d > n_docs) {
            *oob = true;
            return 0;
        }
        return p[d];
    }
};
// eight ids at once where their address is a multiple of 16, as on the device
struct SimTokens {
    const uint32_t* p;
    uint64_t T;
    bool* oob;
    uint32_t one(uint64_t i) const {
        if (i >= T) {
            *oob = true;
            return 0;
        }
        return p[i];
    }
    bool eight(uint64_t i, uint32_t out[8]) const {
        if ((uintptr_t)(p + i) & 15u) return false;
        if (i + 8 > T) {
            *oob = true;
            return false;
        }
        for (int j = 0; j < 8; ++j) out[j] = p[i + j];
        return true;
    }
};
