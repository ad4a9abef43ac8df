/* Stand-in for <fftw3.h> (TEST INFRASTRUCTURE): only the names the reference's wsprd/wsprd.c uses, so that the file
 * compiles where it lies.  The definitions are in fftw3_shim.c; the one transform behind them is the oracle's
 * orc_fft512.  On the include path of the pinned-reference targets of oracle/Makefile only. */
#pragma once
#include <stddef.h>
#include <stdio.h>

typedef float fftwf_complex[2];
typedef struct standin_fftwf_plan *fftwf_plan;

#define FFTW_FORWARD  (-1)
#define FFTW_ESTIMATE (1U << 6)

void      *fftwf_malloc(size_t n);
void       fftwf_free(void *p);
fftwf_plan fftwf_plan_dft_1d(int n, fftwf_complex *in, fftwf_complex *out, int sign, unsigned flags);
void       fftwf_execute(const fftwf_plan plan);
void       fftwf_destroy_plan(fftwf_plan plan);
int        fftwf_import_wisdom_from_file(FILE *f);
void       fftwf_export_wisdom_to_file(FILE *f);
