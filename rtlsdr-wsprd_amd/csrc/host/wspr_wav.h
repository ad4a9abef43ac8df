// RIFF/WAVE reader of wspr_read_wav_file() (include/wspr_mi355x.h).  Plain C++, no HIP: the file is untrusted input.
#pragma once
#include <cstddef>
#include <cstdint>

namespace wspr {
// PCM (format tag 1), 1 channel, 16 bit, 12 000 Hz only.  Returns the samples stored in pcm[0 .. cap), 0 on any error or any
// other format.
size_t read_wav_file(const char* filename, int16_t* pcm, size_t cap);
// The same format, written: 0, or -1 if the file cannot be written (or nsamp does not fit the 32-bit size fields).
int write_wav_file(const char* filename, const int16_t* pcm, size_t nsamp);
}  // namespace wspr
