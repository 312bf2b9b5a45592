// kmer_code.h — what the k-mer kernels of tree_kernels.hip (guide-tree spectra) and dotplot_kernels.hip (window spectra) share: the base code of a
// k-mer character and the number of bits a sort key has in use.
#ifndef CL_KMER_CODE_H
#define CL_KMER_CODE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ uint32_t base_code(uint8_t c) {   // encode_base for ACGTacgt, 4: not a k-mer character
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

inline uint32_t bits_for(uint64_t v) {   // bits needed to hold values 0 .. v (0 for v = 0)
    uint32_t b = 0;
    while (b < 64 && (v >> b) != 0) ++b;
    return b;
}

}  // namespace

#endif
