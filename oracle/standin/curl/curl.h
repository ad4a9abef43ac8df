/* Declaration-only stand-in for <curl/curl.h> (TEST INFRASTRUCTURE): the names the reference's rtlsdr_wsprd.c uses.
 * front_ref_wrap.c defines them to fail; nothing is ever sent. */
#pragma once

typedef void CURL;
typedef enum { CURLE_OK = 0, CURLE_FAILED_INIT = 2 } CURLcode;
typedef enum { CURLOPT_NOBODY = 44, CURLOPT_URL = 10002 } CURLoption;

CURL       *curl_easy_init(void);
CURLcode    curl_easy_setopt(CURL *curl, CURLoption option, ...);
CURLcode    curl_easy_perform(CURL *curl);
void        curl_easy_reset(CURL *curl);
void        curl_easy_cleanup(CURL *curl);
char       *curl_easy_escape(CURL *curl, const char *string, int length);
void        curl_free(void *p);
const char *curl_easy_strerror(CURLcode code);
