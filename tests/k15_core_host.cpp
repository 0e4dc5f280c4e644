// polyfuzz_amd/csrc/k15_core.h -- K15's integer cutoff and block bound -- compiled for the host as a stand-alone program and held
// to the definitions by tests/test_sparse_join_cpu.py.
//   k15_core_host cutoff <in> <out>   in: int32 n, then n x { int32 k; float64 t }.  out: n x int32 smin = k15_cutoff(2^-k, t).
//       The program itself checks the definition -- smin passes, smin - 1 does not (smin == 1: nothing below it counts;
//       smin == 0: not even 2^31 - 1 passes) -- and exits 1 when it is violated; the test checks it again in numpy.
//   k15_core_host bound <in> <out>    in: float32 max_norm, int32 n, then n x { int32 count; count x float32 as_k }.
//       out: n x float32 k15_block_bound(mass, max_norm), mass = the float32 sum of as_k^2 in the order given.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <vector>

#include "../polyfuzz_amd/csrc/k15_core.h"

using namespace pfz;

template <class T> static bool get(FILE *f, T *v) { return fread(v, sizeof(T), 1, f) == 1; }

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int bad = 0;
    if (!strcmp(argv[1], "cutoff")) {
        int32_t n = 0;
        if (!get(in, &n)) return 2;
        for (int32_t i = 0; i < n; ++i) {
            int32_t k;
            double t;
            if (!get(in, &k) || !get(in, &t)) return 2;
            const float inv_scale = (float)ldexp(1.0, -k);
            const int32_t smin = k15_cutoff(inv_scale, t);
            if (smin == 0) bad += k15_passes(INT32_MAX, inv_scale, t);
            else bad += !k15_passes(smin, inv_scale, t) || (smin > 1 && k15_passes(smin - 1, inv_scale, t));
            fwrite(&smin, sizeof(smin), 1, out);
        }
    } else if (!strcmp(argv[1], "bound")) {
        float max_norm;
        int32_t n = 0;
        if (!get(in, &max_norm) || !get(in, &n)) return 2;
        std::vector<float> v;
        for (int32_t i = 0; i < n; ++i) {
            int32_t count;
            if (!get(in, &count) || count < 0 || count > 64) return 2;
            v.resize((size_t)count);
            if (count && fread(v.data(), sizeof(float), (size_t)count, in) != (size_t)count) return 2;
            float mass = 0.f;
            for (float x : v) mass += x * x;
            const float b = k15_block_bound(mass, max_norm);
            fwrite(&b, sizeof(b), 1, out);
        }
    } else {
        return 2;
    }
    fclose(out);
    fclose(in);
    if (bad) fprintf(stderr, "k15_core_host: %d cutoffs violate their definition\n", bad);
    return bad ? 1 : 0;
}
