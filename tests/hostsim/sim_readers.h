// How the CPU simulations of the row, padded and samples passes (rows_sim.cpp, padded_sim.cpp, samples_sim.cpp) hand arrays to the
// functions they share with the kernels: every index is checked, and one out of bounds sets *oob instead of being read.
#pragma once
#include <stdint.h>

#include <utility>

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
// entries [0, n) of an array
template <class T>
struct SimArray {
    const T* p;
    uint64_t n;
    bool* oob;
    T operator[](uint64_t i) const {
        if (i >= n) {
            *oob = true;
            return 0;
        }
        return p[i];
    }
};
// what a scan kernel leaves (tk_scan_blocks<false>): exclusive sums in place; returns the total
template <class T>
uint64_t sim_scan(T* a, uint64_t n) {
    uint64_t carry = 0;
    for (uint64_t i = 0; i < n; ++i) carry += std::exchange(a[i], (T)carry);  // (a[i] = the sum before it; its count joins the sum)
    return carry;
}
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
