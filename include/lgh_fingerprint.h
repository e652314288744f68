/* lgh_fingerprint.h — the state fingerprint: one function for host and device.
 *
 * A position-sensitive 128-bit fingerprint of a sequence of 64-bit words w_i (the bit pattern of a double, or an integer
 * widened to 64 bits) at positions i = offset + k:
 *
 *    h_i   = mix(w_i + (i + 1) * 0x9E3779B97F4A7C15)                       (mod 2^64)
 *    fp[0] = sum of the h_i (mod 2^64),   fp[1] = xor of the h_i
 *
 * with mix = the finaliser of splitmix64.  Both words are associative and commutative in the h_i: the result does not
 * depend on the order in which a kernel, a host loop or several ranks take the words, and the fingerprint of a
 * concatenation is the word-wise combination (add, xor) of the fingerprints of its parts, each taken at its offset.
 * -0.0, NaN payloads and denormals count as the bits they are.
 *
 * Plain C; __host__ __device__ under HIP.  The kernel (laghos_amd/csrc/lgh_fingerprint.hip), lgh_fingerprint_host and
 * the checkpoint code (laghos_amd/host/checkpoint.cpp) all include this file: there is one definition.
 */
#ifndef LGH_FINGERPRINT_H
#define LGH_FINGERPRINT_H

#if defined(__HIPCC__)
#define LGH_FP_FN __host__ __device__ static inline
#else
#define LGH_FP_FN static inline
#endif

#define LGH_FP_GOLDEN 0x9E3779B97F4A7C15ULL

LGH_FP_FN unsigned long long lgh_fp_mix(unsigned long long z)
{
   z ^= z >> 30;
   z *= 0xBF58476D1CE4E5B9ULL;
   z ^= z >> 27;
   z *= 0x94D049BB133111EBULL;
   z ^= z >> 31;
   return z;
}

/* h_i of word w at position i */
LGH_FP_FN unsigned long long lgh_fp_word(unsigned long long w, unsigned long long i)
{
   return lgh_fp_mix(w + (i + 1ULL) * LGH_FP_GOLDEN);
}

/* fp := fp combined with the n words at `words`, the first of them at position `offset` (host loop) */
static inline void lgh_fp_accumulate(const unsigned long long *words, long n, unsigned long long offset, unsigned long long fp[2])
{
   unsigned long long s = fp[0], x = fp[1];
   long k;
   for (k = 0; k < n; k++)
   {
      const unsigned long long h = lgh_fp_word(words[k], offset + (unsigned long long)k);
      s += h;
      x ^= h;
   }
   fp[0] = s;
   fp[1] = x;
}

#endif /* LGH_FINGERPRINT_H */
