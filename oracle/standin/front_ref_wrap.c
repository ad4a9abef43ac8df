/* The reference receiver's translation unit, compiled where it lies (TEST INFRASTRUCTURE).  Its decimator callback and
 * its state are file-local, so this wrapper includes the file and exports a feeder and a reader beside it.  The
 * rtl-sdr and curl functions it names are defined here to fail; main is renamed and never called. */
#include <stdint.h>
#include <string.h>

#include "rtl-sdr.h"
#include "curl/curl.h"

#define main ref_rtlsdr_main
#include "rtlsdr_wsprd.c"
#undef main

/* one callback's worth of interleaved u8 IQ; the callback rewrites buf in place */
void front_ref_feed(unsigned char *buf, uint32_t nbytes) { rtlsdr_callback(buf, nbytes, NULL); }

/* outputs so far in the buffer being filled */
uint32_t front_ref_count(void) { return rx_state.iqIndex[rx_state.bufferIndex]; }

/* copy out the first n outputs (n <= front_ref_count()) */
void front_ref_read(float *I, float *Q, uint32_t n) {
    uint32_t idx = rx_state.bufferIndex;
    memcpy(I, rx_state.iSamples[idx], (size_t)n * sizeof(float));
    memcpy(Q, rx_state.qSamples[idx], (size_t)n * sizeof(float));
}

uint32_t    rtlsdr_get_device_count(void) { return 0; }
const char *rtlsdr_get_device_name(uint32_t index) { (void)index; return ""; }
int rtlsdr_get_device_usb_strings(uint32_t i, char *m, char *p, char *s) { (void)i; (void)m; (void)p; (void)s; return -1; }
int rtlsdr_open(rtlsdr_dev_t **dev, uint32_t index) { (void)dev; (void)index; return -1; }
int rtlsdr_close(rtlsdr_dev_t *dev) { (void)dev; return -1; }
int rtlsdr_set_center_freq(rtlsdr_dev_t *dev, uint32_t freq) { (void)dev; (void)freq; return -1; }
int rtlsdr_set_freq_correction(rtlsdr_dev_t *dev, int ppm) { (void)dev; (void)ppm; return -1; }
int rtlsdr_set_tuner_gain(rtlsdr_dev_t *dev, int gain) { (void)dev; (void)gain; return -1; }
int rtlsdr_set_tuner_gain_mode(rtlsdr_dev_t *dev, int manual) { (void)dev; (void)manual; return -1; }
int rtlsdr_set_sample_rate(rtlsdr_dev_t *dev, uint32_t rate) { (void)dev; (void)rate; return -1; }
int rtlsdr_set_direct_sampling(rtlsdr_dev_t *dev, int on) { (void)dev; (void)on; return -1; }
int rtlsdr_reset_buffer(rtlsdr_dev_t *dev) { (void)dev; return -1; }
int rtlsdr_read_async(rtlsdr_dev_t *dev, rtlsdr_read_async_cb_t cb, void *ctx, uint32_t n, uint32_t len) {
    (void)dev; (void)cb; (void)ctx; (void)n; (void)len; return -1;
}
int rtlsdr_cancel_async(rtlsdr_dev_t *dev) { (void)dev; return -1; }

CURL       *curl_easy_init(void) { return NULL; }
CURLcode    curl_easy_setopt(CURL *curl, CURLoption option, ...) { (void)curl; (void)option; return CURLE_FAILED_INIT; }
CURLcode    curl_easy_perform(CURL *curl) { (void)curl; return CURLE_FAILED_INIT; }
void        curl_easy_reset(CURL *curl) { (void)curl; }
void        curl_easy_cleanup(CURL *curl) { (void)curl; }
char       *curl_easy_escape(CURL *curl, const char *s, int n) { (void)curl; (void)s; (void)n; return NULL; }
void        curl_free(void *p) { (void)p; }
const char *curl_easy_strerror(CURLcode code) { (void)code; return "curl stand-in: nothing is sent"; }
