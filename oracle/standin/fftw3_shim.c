/* Definitions behind the <fftw3.h> stand-in (TEST INFRASTRUCTURE).  A plan remembers its in and out pointers; execute
 * runs the oracle's 512-point forward FFT on them.  Any other request aborts: nothing here may quietly compute a
 * transform the oracle does not have.  Wisdom is a no-op (the caller still creates its empty fftw_wisdom.dat). */
#include "fftw3.h"

#include <stdlib.h>

#include "wspr_oracle.h"

struct standin_fftwf_plan { fftwf_complex *in, *out; };

void *fftwf_malloc(size_t n) { return malloc(n); }
void  fftwf_free(void *p) { free(p); }

fftwf_plan fftwf_plan_dft_1d(int n, fftwf_complex *in, fftwf_complex *out, int sign, unsigned flags) {
    (void)flags;
    if (n != ORC_FFT || sign != FFTW_FORWARD || !in || !out) abort();
    fftwf_plan p = (fftwf_plan)malloc(sizeof *p);
    if (!p) abort();
    p->in = in;
    p->out = out;
    return p;
}

void fftwf_execute(const fftwf_plan p) {
    float re[ORC_FFT], im[ORC_FFT];
    if (!p) abort();
    for (int j = 0; j < ORC_FFT; j++) { re[j] = p->in[j][0]; im[j] = p->in[j][1]; }
    orc_fft512(re, im);
    for (int j = 0; j < ORC_FFT; j++) { p->out[j][0] = re[j]; p->out[j][1] = im[j]; }
}

void fftwf_destroy_plan(fftwf_plan p) { free(p); }
int  fftwf_import_wisdom_from_file(FILE *f) { (void)f; return 0; }
void fftwf_export_wisdom_to_file(FILE *f) { (void)f; }
