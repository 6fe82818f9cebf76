/* The seven coarsest-matrix entry points of csrc/mg3d_host.c under the host sanitizers, as a program of its own:
 *   gcc -std=gnu99 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
 *       tools/coarse_matrix_asan.c multigrid_parallel_amd/csrc/mg3d_host.c -lm -o /tmp/coarse_matrix_asan && /tmp/coarse_matrix_asan
 * Every matrix is an exact calloc of N^6 doubles, eps and mask exact N^3 arrays, so a row or a neighbour index outside
 * the matrix or the fields is a report.  Cases: tests/test_mask_host.py's boundaries at N = 3, 5, 9 (a periodic axis
 * needs N - 1 >= 4), sigma 0 and 3.5, constant and eps, masks none / all-zero / sparse / dense; the screening field of
 * mg3d_coarse_matrix_field is an exact N^3 array too, zero where the mask's byte is (all zero: the pin's scan runs through). */
#include <stdio.h>
#include <stdlib.h>

#include "mg3d.h"

static const int BCS[][2] = {{0, 0}, {5, 0}, {0, 10}, {4, 3}, {7, 0}, {0, 63}, {2, 51}};

int main(void)
{
    int cases = 0;
    unsigned seed = 12345u;
    for (int N = 3; N <= 9; N = 2 * N - 1) {
        const size_t n = (size_t)N * N * N;
        double *eps = (double *)malloc(n * sizeof(double));
        unsigned char *mask = (unsigned char *)malloc(n);
        double *fld = (double *)malloc(n * sizeof(double));
        for (size_t p = 0; p < n; p++)
            eps[p] = 0.5 + (double)((seed = seed * 1664525u + 1013904223u) >> 8) / (1u << 24) * 3.5;
        for (int sg = 0; sg < 2; sg++)
            for (int ef = 0; ef < 2; ef++)
                for (size_t b = 0; b < sizeof BCS / sizeof BCS[0]; b++)
                    for (int density = -1; density < 3; density++) { /* -1: NULL, 0: all zero, 1: 10 %, 2: 50 % */
                        const int axes = BCS[b][0], faces = BCS[b][1];
                        const double sigma = sg ? 3.5 : 0., h = 0.125, *e = ef ? eps : NULL;
                        if (axes && N - 1 < 4)
                            continue;
                        for (size_t p = 0; p < n; p++) {
                            const unsigned r = (seed = seed * 1664525u + 1013904223u) >> 16;
                            mask[p] = (density == 1 && r % 10 == 0) || (density == 2 && r % 2 == 0) ? 1 + r % 255 : 0;
                            fld[p] = mask[p] * 0.25;
                        }
                        for (int entry = 0; entry < 7; entry++) {
                            double *A = (double *)calloc(n * n, sizeof(double));
                            if (!A)
                                return 2;
                            switch (entry) {
                            case 0: mg3d_coarse_matrix(A, N, h); break;
                            case 1: mg3d_coarse_matrix_shift(A, N, h, sigma); break;
                            case 2: mg3d_coarse_matrix_coef(A, N, h, eps, sigma); break;
                            case 3: mg3d_coarse_matrix_periodic(A, N, h, e, sigma, axes); break;
                            case 4: mg3d_coarse_matrix_bc(A, N, h, e, sigma, axes, faces); break;
                            case 5: mg3d_coarse_matrix_mask(A, N, h, e, sigma, axes, faces, density < 0 ? NULL : mask); break;
                            default: mg3d_coarse_matrix_field(A, N, h, e, sigma, axes, faces, density == 2 ? mask : NULL, density < 0 ? NULL : fld);
                            }
                            double tr = 0.; /* (every row has its diagonal: read the whole matrix once) */
                            for (size_t p = 0; p < n; p++)
                                tr += A[p * n + p];
                            if (tr != tr)
                                return 3;
                            free(A);
                            cases++;
                        }
                    }
        free(eps);
        free(mask);
        free(fld);
    }
    printf("coarse_matrix_asan: %d calls, clean\n", cases);
    return 0;
}
