// The atomics of the region kernels that the test emulator (tests/emu) does not supply: it runs one thread at a time and has atomicAdd
// on 32-bit words only, so each of these is a plain read-modify-write.  A device build sees nothing of this file.
#pragma once
#include "tsii_common.h"

#ifdef TSII_HIP_EMU
namespace tsii {

static inline int atomicMin(int* p, int v) { const int o = *p; if (v < o) *p = v; return o; }
static inline unsigned atomicMin(unsigned* p, unsigned v) { const unsigned o = *p; if (v < o) *p = v; return o; }
static inline int atomicMax(int* p, int v) { const int o = *p; if (v > o) *p = v; return o; }
static inline int atomicCAS(int* p, int expect, int v) { const int o = *p; if (o == expect) *p = v; return o; }
using ::atomicAdd;                               // the overload below would hide the emulator's own
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; *p = o + v; return o; }
static inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; if (v > o) *p = v; return o; }

}  // namespace tsii
#endif
