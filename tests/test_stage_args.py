"""The stage calls' argument checks (rtlsdr-wsprd_amd/csrc/host/wspr_stage_args.h), without a device: the stand-alone program
tests/helpers/stage_args_check.cpp runs a fixed table of calls through them and prints, per case, the code and the line
on stderr.  EXPECTED is what the entry points of the library themselves answered to these calls before the checks were
gathered in that header (recorded on a machine without a GPU, where a call that passes every check fails only when it
asks for a device: those are the lines with code 0 and no text).  It holds every text of the header for every entry
point that can produce it, and the cases in which two things are wrong and the order of the checks picks the line and
the code: a record that is too long and misaligned (-2, not -1), a negative count with a null pointer, no segments with
bad pointers (accepted), a list that breaks two limits, K8 against K17 on 900 Hz, a negative sigma and flag bit 2.
Not reachable: "list not sorted by seg" from wspr_synth(), wspr_synth_faded() and wspr_synth_audio(), whose one segment
leaves a list no way of being out of order without a seg outside the batch, which is tested first.
The second test runs the same program under AddressSanitizer and UBSan."""
import os
import subprocess

import oracle_lib as ol

_SRC = os.path.join(ol.ROOT, "tests", "helpers", "stage_args_check.cpp")
_FLAGS = ["-std=c++17", "-Wall", "-I", os.path.join(ol.ROOT, "rtlsdr-wsprd_amd", "csrc", "host")]

EXPECTED = """\
wspr_synth_batch_device/fine 0 |
wspr_synth_batch_device/empty_list_null 0 |
wspr_synth_batch_device/ntx_negative_and_null_list -1 |libwspr_mi355x: wspr_synth_batch_device: negative count
wspr_synth_batch_device/no_list -1 |libwspr_mi355x: wspr_synth_batch_device: no transmission list
wspr_synth_batch_device/sigma_nan -1 |libwspr_mi355x: wspr_synth_batch_device: noise_sigma is not finite
wspr_synth_batch_device/sigma_negative 0 |
wspr_synth_batch_device/sigma_negative_and_flag_bit_4 -1 |libwspr_mi355x: wspr_synth_batch_device: unknown flag bit
wspr_synth_batch_device/sigma_2e6 0 |
wspr_synth_batch_device/flag_bit_2 0 |
wspr_synth_batch_device/flag_bit_4 -1 |libwspr_mi355x: wspr_synth_batch_device: unknown flag bit
wspr_synth_batch_device/seg_negative -1 |libwspr_mi355x: wspr_synth_batch_device: transmission 0: seg outside the batch
wspr_synth_batch_device/seg_outside -1 |libwspr_mi355x: wspr_synth_batch_device: transmission 0: seg outside the batch
wspr_synth_batch_device/unsorted -1 |libwspr_mi355x: wspr_synth_batch_device: transmission 1: list not sorted by seg
wspr_synth_batch_device/f0_nan -1 |libwspr_mi355x: wspr_synth_batch_device: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_batch_device/drift_inf -1 |libwspr_mi355x: wspr_synth_batch_device: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_batch_device/amp_2e6 0 |
wspr_synth_batch_device/amp_2e6_and_900_hz 0 |
wspr_synth_batch_device/900_hz 0 |
wspr_synth_batch_device/700_hz_and_drift_300 0 |
wspr_synth_batch_device/1100_hz -1 |libwspr_mi355x: wspr_synth_batch_device: transmission 0: |f0| + |drift|/2 above 1000 Hz
wspr_synth_batch_device/symbol_4_in_second -1 |libwspr_mi355x: wspr_synth_batch_device: transmission 1: channel symbol above 3
wspr_synth_batch_device/nseg_negative -1 |libwspr_mi355x: wspr_synth_batch_device: negative count
wspr_synth_batch_device/nseg_0_and_bad_rows 0 |
wspr_synth_batch_device/no_i -1 |libwspr_mi355x: wspr_synth_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_synth_batch_device/no_q -1 |libwspr_mi355x: wspr_synth_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_synth_batch_device/q_misaligned -1 |libwspr_mi355x: wspr_synth_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_synth_batch_device/flag_bit_4_and_q_misaligned -1 |libwspr_mi355x: wspr_synth_batch_device: unknown flag bit
wspr_synth_faded_batch_device/fine 0 |
wspr_synth_faded_batch_device/empty_list_null 0 |
wspr_synth_faded_batch_device/ntx_negative_and_null_list -1 |libwspr_mi355x: wspr_synth_faded_batch_device: negative count
wspr_synth_faded_batch_device/no_list -1 |libwspr_mi355x: wspr_synth_faded_batch_device: no transmission list
wspr_synth_faded_batch_device/sigma_nan -1 |libwspr_mi355x: wspr_synth_faded_batch_device: noise_sigma is not finite
wspr_synth_faded_batch_device/sigma_negative 0 |
wspr_synth_faded_batch_device/sigma_negative_and_flag_bit_4 -1 |libwspr_mi355x: wspr_synth_faded_batch_device: unknown flag bit
wspr_synth_faded_batch_device/sigma_2e6 0 |
wspr_synth_faded_batch_device/flag_bit_2 0 |
wspr_synth_faded_batch_device/flag_bit_4 -1 |libwspr_mi355x: wspr_synth_faded_batch_device: unknown flag bit
wspr_synth_faded_batch_device/seg_negative -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0: seg outside the batch
wspr_synth_faded_batch_device/seg_outside -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0: seg outside the batch
wspr_synth_faded_batch_device/unsorted -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 1: list not sorted by seg
wspr_synth_faded_batch_device/f0_nan -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_faded_batch_device/drift_inf -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_faded_batch_device/amp_2e6 0 |
wspr_synth_faded_batch_device/amp_2e6_and_900_hz 0 |
wspr_synth_faded_batch_device/900_hz 0 |
wspr_synth_faded_batch_device/700_hz_and_drift_300 0 |
wspr_synth_faded_batch_device/1100_hz -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0: |f0| + |drift|/2 above 1000 Hz
wspr_synth_faded_batch_device/symbol_4_in_second -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 1: channel symbol above 3
wspr_synth_faded_batch_device/nseg_negative -1 |libwspr_mi355x: wspr_synth_faded_batch_device: negative count
wspr_synth_faded_batch_device/nseg_0_and_bad_rows 0 |
wspr_synth_faded_batch_device/no_i -1 |libwspr_mi355x: wspr_synth_faded_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_synth_faded_batch_device/no_q -1 |libwspr_mi355x: wspr_synth_faded_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_synth_faded_batch_device/q_misaligned -1 |libwspr_mi355x: wspr_synth_faded_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_synth_faded_batch_device/flag_bit_4_and_q_misaligned -1 |libwspr_mi355x: wspr_synth_faded_batch_device: unknown flag bit
wspr_synth_faded_batch_device/channel_fine 0 |
wspr_synth_faded_batch_device/channel_no_channels 0 |
wspr_synth_faded_batch_device/channel_gain_nan -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0, path 0: gain, shift or sigma is not finite
wspr_synth_faded_batch_device/channel_sigma_20 -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0, path 1: sigma neither 0 nor within 0.001 .. 10 Hz
wspr_synth_faded_batch_device/channel_sigma_1e-4 -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0, path 0: sigma neither 0 nor within 0.001 .. 10 Hz
wspr_synth_faded_batch_device/channel_sigma_negative -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0, path 0: sigma neither 0 nor within 0.001 .. 10 Hz
wspr_synth_faded_batch_device/channel_shift_200 -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0, path 1: |shift| above 100 Hz
wspr_synth_faded_batch_device/channel_sigma_20_and_shift_200 -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0, path 0: sigma neither 0 nor within 0.001 .. 10 Hz
wspr_synth_faded_batch_device/channel_sigma_20_and_q_misaligned -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0, path 1: sigma neither 0 nor within 0.001 .. 10 Hz
wspr_synth_faded_batch_device/1100_hz_and_channel_sigma_20 -1 |libwspr_mi355x: wspr_synth_faded_batch_device: transmission 0: |f0| + |drift|/2 above 1000 Hz
wspr_synth/fine 0 |
wspr_synth/empty_list_null 0 |
wspr_synth/ntx_negative_and_null_list -1 |libwspr_mi355x: wspr_synth: negative count
wspr_synth/no_list -1 |libwspr_mi355x: wspr_synth: no transmission list
wspr_synth/sigma_nan -1 |libwspr_mi355x: wspr_synth: noise_sigma is not finite
wspr_synth/sigma_negative 0 |
wspr_synth/sigma_negative_and_flag_bit_4 -1 |libwspr_mi355x: wspr_synth: unknown flag bit
wspr_synth/sigma_2e6 0 |
wspr_synth/flag_bit_2 0 |
wspr_synth/flag_bit_4 -1 |libwspr_mi355x: wspr_synth: unknown flag bit
wspr_synth/seg_negative -1 |libwspr_mi355x: wspr_synth: transmission 0: seg outside the batch
wspr_synth/seg_outside -1 |libwspr_mi355x: wspr_synth: transmission 0: seg outside the batch
wspr_synth/unsorted -1 |libwspr_mi355x: wspr_synth: transmission 1: seg outside the batch
wspr_synth/f0_nan -1 |libwspr_mi355x: wspr_synth: transmission 0: f0, t0, amp or drift is not finite
wspr_synth/drift_inf -1 |libwspr_mi355x: wspr_synth: transmission 0: f0, t0, amp or drift is not finite
wspr_synth/amp_2e6 0 |
wspr_synth/amp_2e6_and_900_hz 0 |
wspr_synth/900_hz 0 |
wspr_synth/700_hz_and_drift_300 0 |
wspr_synth/1100_hz -1 |libwspr_mi355x: wspr_synth: transmission 0: |f0| + |drift|/2 above 1000 Hz
wspr_synth/symbol_4_in_second -1 |libwspr_mi355x: wspr_synth: transmission 1: channel symbol above 3
wspr_synth/no_i -1 |libwspr_mi355x: wspr_synth: no output rows
wspr_synth/no_q -1 |libwspr_mi355x: wspr_synth: no output rows
wspr_synth_faded/fine 0 |
wspr_synth_faded/empty_list_null 0 |
wspr_synth_faded/ntx_negative_and_null_list -1 |libwspr_mi355x: wspr_synth_faded: negative count
wspr_synth_faded/no_list -1 |libwspr_mi355x: wspr_synth_faded: no transmission list
wspr_synth_faded/sigma_nan -1 |libwspr_mi355x: wspr_synth_faded: noise_sigma is not finite
wspr_synth_faded/sigma_negative 0 |
wspr_synth_faded/sigma_negative_and_flag_bit_4 -1 |libwspr_mi355x: wspr_synth_faded: unknown flag bit
wspr_synth_faded/sigma_2e6 0 |
wspr_synth_faded/flag_bit_2 0 |
wspr_synth_faded/flag_bit_4 -1 |libwspr_mi355x: wspr_synth_faded: unknown flag bit
wspr_synth_faded/seg_negative -1 |libwspr_mi355x: wspr_synth_faded: transmission 0: seg outside the batch
wspr_synth_faded/seg_outside -1 |libwspr_mi355x: wspr_synth_faded: transmission 0: seg outside the batch
wspr_synth_faded/unsorted -1 |libwspr_mi355x: wspr_synth_faded: transmission 1: seg outside the batch
wspr_synth_faded/f0_nan -1 |libwspr_mi355x: wspr_synth_faded: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_faded/drift_inf -1 |libwspr_mi355x: wspr_synth_faded: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_faded/amp_2e6 0 |
wspr_synth_faded/amp_2e6_and_900_hz 0 |
wspr_synth_faded/900_hz 0 |
wspr_synth_faded/700_hz_and_drift_300 0 |
wspr_synth_faded/1100_hz -1 |libwspr_mi355x: wspr_synth_faded: transmission 0: |f0| + |drift|/2 above 1000 Hz
wspr_synth_faded/symbol_4_in_second -1 |libwspr_mi355x: wspr_synth_faded: transmission 1: channel symbol above 3
wspr_synth_faded/no_i -1 |libwspr_mi355x: wspr_synth_faded: no output rows
wspr_synth_faded/no_q -1 |libwspr_mi355x: wspr_synth_faded: no output rows
wspr_synth_faded/channel_fine 0 |
wspr_synth_faded/channel_no_channels 0 |
wspr_synth_faded/channel_gain_nan -1 |libwspr_mi355x: wspr_synth_faded: transmission 0, path 0: gain, shift or sigma is not finite
wspr_synth_faded/channel_sigma_20 -1 |libwspr_mi355x: wspr_synth_faded: transmission 0, path 1: sigma neither 0 nor within 0.001 .. 10 Hz
wspr_synth_faded/channel_sigma_1e-4 -1 |libwspr_mi355x: wspr_synth_faded: transmission 0, path 0: sigma neither 0 nor within 0.001 .. 10 Hz
wspr_synth_faded/channel_sigma_negative -1 |libwspr_mi355x: wspr_synth_faded: transmission 0, path 0: sigma neither 0 nor within 0.001 .. 10 Hz
wspr_synth_faded/channel_shift_200 -1 |libwspr_mi355x: wspr_synth_faded: transmission 0, path 1: |shift| above 100 Hz
wspr_synth_faded/channel_sigma_20_and_shift_200 -1 |libwspr_mi355x: wspr_synth_faded: transmission 0, path 0: sigma neither 0 nor within 0.001 .. 10 Hz
wspr_synth_audio_batch_device/fine 0 |
wspr_synth_audio_batch_device/empty_list_null 0 |
wspr_synth_audio_batch_device/ntx_negative_and_null_list -1 |libwspr_mi355x: wspr_synth_audio_batch_device: negative count
wspr_synth_audio_batch_device/no_list -1 |libwspr_mi355x: wspr_synth_audio_batch_device: no transmission list
wspr_synth_audio_batch_device/sigma_nan -1 |libwspr_mi355x: wspr_synth_audio_batch_device: noise_sigma is not finite
wspr_synth_audio_batch_device/sigma_negative -1 |libwspr_mi355x: wspr_synth_audio_batch_device: noise_sigma is negative
wspr_synth_audio_batch_device/sigma_negative_and_flag_bit_4 -1 |libwspr_mi355x: wspr_synth_audio_batch_device: noise_sigma is negative
wspr_synth_audio_batch_device/sigma_2e6 -1 |libwspr_mi355x: wspr_synth_audio_batch_device: noise_sigma above 1e6
wspr_synth_audio_batch_device/flag_bit_2 -1 |libwspr_mi355x: wspr_synth_audio_batch_device: unknown flag bit
wspr_synth_audio_batch_device/flag_bit_4 -1 |libwspr_mi355x: wspr_synth_audio_batch_device: unknown flag bit
wspr_synth_audio_batch_device/seg_negative -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 0: seg outside the batch
wspr_synth_audio_batch_device/seg_outside -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 0: seg outside the batch
wspr_synth_audio_batch_device/unsorted -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 1: list not sorted by seg
wspr_synth_audio_batch_device/f0_nan -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_audio_batch_device/drift_inf -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_audio_batch_device/amp_2e6 -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 0: |amp| above 1e6
wspr_synth_audio_batch_device/amp_2e6_and_900_hz -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 0: |amp| above 1e6
wspr_synth_audio_batch_device/900_hz -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 0: |f0| + |drift|/2 above 800 Hz
wspr_synth_audio_batch_device/700_hz_and_drift_300 -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 0: |f0| + |drift|/2 above 800 Hz
wspr_synth_audio_batch_device/1100_hz -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 0: |f0| + |drift|/2 above 800 Hz
wspr_synth_audio_batch_device/symbol_4_in_second -1 |libwspr_mi355x: wspr_synth_audio_batch_device: transmission 1: channel symbol above 3
wspr_synth_audio_batch_device/nseg_negative -1 |libwspr_mi355x: wspr_synth_audio_batch_device: negative count
wspr_synth_audio_batch_device/nsamp_negative_and_no_pcm -1 |libwspr_mi355x: wspr_synth_audio_batch_device: negative count
wspr_synth_audio_batch_device/nsamp_1440000 0 |
wspr_synth_audio_batch_device/nsamp_1440001 -2 |libwspr_mi355x: wspr_synth_audio_batch_device: a record holds at most 1440000 samples (120 s)
wspr_synth_audio_batch_device/nsamp_1440001_and_pcm_misaligned -2 |libwspr_mi355x: wspr_synth_audio_batch_device: a record holds at most 1440000 samples (120 s)
wspr_synth_audio_batch_device/nsamp_1440001_and_sigma_nan -2 |libwspr_mi355x: wspr_synth_audio_batch_device: a record holds at most 1440000 samples (120 s)
wspr_synth_audio_batch_device/nseg_0_and_bad_pcm 0 |
wspr_synth_audio_batch_device/no_pcm -1 |libwspr_mi355x: wspr_synth_audio_batch_device: d_pcm must be 16-byte aligned device memory
wspr_synth_audio_batch_device/pcm_misaligned -1 |libwspr_mi355x: wspr_synth_audio_batch_device: d_pcm must be 16-byte aligned device memory
wspr_synth_audio_batch_device/pcm_misaligned_and_stride_odd -1 |libwspr_mi355x: wspr_synth_audio_batch_device: d_pcm must be 16-byte aligned device memory
wspr_synth_audio_batch_device/stride_1004 -1 |libwspr_mi355x: wspr_synth_audio_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_synth_audio_batch_device/stride_992 -1 |libwspr_mi355x: wspr_synth_audio_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_synth_audio_batch_device/flag_bit_2_and_stride_992 -1 |libwspr_mi355x: wspr_synth_audio_batch_device: unknown flag bit
wspr_synth_audio/fine 0 |
wspr_synth_audio/empty_list_null 0 |
wspr_synth_audio/ntx_negative_and_null_list -1 |libwspr_mi355x: wspr_synth_audio: negative count
wspr_synth_audio/no_list -1 |libwspr_mi355x: wspr_synth_audio: no transmission list
wspr_synth_audio/sigma_nan -1 |libwspr_mi355x: wspr_synth_audio: noise_sigma is not finite
wspr_synth_audio/sigma_negative -1 |libwspr_mi355x: wspr_synth_audio: noise_sigma is negative
wspr_synth_audio/sigma_negative_and_flag_bit_4 -1 |libwspr_mi355x: wspr_synth_audio: noise_sigma is negative
wspr_synth_audio/sigma_2e6 -1 |libwspr_mi355x: wspr_synth_audio: noise_sigma above 1e6
wspr_synth_audio/flag_bit_2 -1 |libwspr_mi355x: wspr_synth_audio: unknown flag bit
wspr_synth_audio/flag_bit_4 -1 |libwspr_mi355x: wspr_synth_audio: unknown flag bit
wspr_synth_audio/seg_negative -1 |libwspr_mi355x: wspr_synth_audio: transmission 0: seg outside the batch
wspr_synth_audio/seg_outside -1 |libwspr_mi355x: wspr_synth_audio: transmission 0: seg outside the batch
wspr_synth_audio/unsorted -1 |libwspr_mi355x: wspr_synth_audio: transmission 1: seg outside the batch
wspr_synth_audio/f0_nan -1 |libwspr_mi355x: wspr_synth_audio: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_audio/drift_inf -1 |libwspr_mi355x: wspr_synth_audio: transmission 0: f0, t0, amp or drift is not finite
wspr_synth_audio/amp_2e6 -1 |libwspr_mi355x: wspr_synth_audio: transmission 0: |amp| above 1e6
wspr_synth_audio/amp_2e6_and_900_hz -1 |libwspr_mi355x: wspr_synth_audio: transmission 0: |amp| above 1e6
wspr_synth_audio/900_hz -1 |libwspr_mi355x: wspr_synth_audio: transmission 0: |f0| + |drift|/2 above 800 Hz
wspr_synth_audio/700_hz_and_drift_300 -1 |libwspr_mi355x: wspr_synth_audio: transmission 0: |f0| + |drift|/2 above 800 Hz
wspr_synth_audio/1100_hz -1 |libwspr_mi355x: wspr_synth_audio: transmission 0: |f0| + |drift|/2 above 800 Hz
wspr_synth_audio/symbol_4_in_second -1 |libwspr_mi355x: wspr_synth_audio: transmission 1: channel symbol above 3
wspr_synth_audio/nsamp_negative -1 |libwspr_mi355x: wspr_synth_audio: negative count
wspr_synth_audio/nsamp_1440001_and_no_record -2 |libwspr_mi355x: wspr_synth_audio: a record holds at most 1440000 samples (120 s)
wspr_synth_audio/no_record -1 |libwspr_mi355x: wspr_synth_audio: no output record
wspr_synth_audio/nsamp_0_and_no_record 0 |
wspr_audio_batch_device/fine 0 |
wspr_audio_batch_device/nseg_negative_and_no_pcm -1 |libwspr_mi355x: wspr_audio_batch_device: negative count
wspr_audio_batch_device/nsamp_negative -1 |libwspr_mi355x: wspr_audio_batch_device: negative count
wspr_audio_batch_device/nsamp_1440000 0 |
wspr_audio_batch_device/nsamp_1440001 -2 |libwspr_mi355x: wspr_audio_batch_device: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_batch_device/nsamp_1440001_and_pcm_misaligned -2 |libwspr_mi355x: wspr_audio_batch_device: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_batch_device/nsamp_1440001_and_nseg_0 -2 |libwspr_mi355x: wspr_audio_batch_device: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_batch_device/nseg_0_and_bad_pointers 0 |
wspr_audio_batch_device/no_pcm -1 |libwspr_mi355x: wspr_audio_batch_device: d_pcm must be 16-byte aligned device memory
wspr_audio_batch_device/pcm_misaligned -1 |libwspr_mi355x: wspr_audio_batch_device: d_pcm must be 16-byte aligned device memory
wspr_audio_batch_device/stride_1004 -1 |libwspr_mi355x: wspr_audio_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_audio_batch_device/stride_992 -1 |libwspr_mi355x: wspr_audio_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_audio_batch_device/stride_992_and_no_rows -1 |libwspr_mi355x: wspr_audio_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_audio_batch_device/no_i -1 |libwspr_mi355x: wspr_audio_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_audio_batch_device/no_q -1 |libwspr_mi355x: wspr_audio_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_audio_batch_device/i_misaligned -1 |libwspr_mi355x: wspr_audio_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_audio_blanked_batch_device/fine 0 |
wspr_audio_blanked_batch_device/nseg_negative_and_no_pcm -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: negative count
wspr_audio_blanked_batch_device/nsamp_negative -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: negative count
wspr_audio_blanked_batch_device/nsamp_1440000 0 |
wspr_audio_blanked_batch_device/nsamp_1440001 -2 |libwspr_mi355x: wspr_audio_blanked_batch_device: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_blanked_batch_device/nsamp_1440001_and_pcm_misaligned -2 |libwspr_mi355x: wspr_audio_blanked_batch_device: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_blanked_batch_device/nsamp_1440001_and_nseg_0 -2 |libwspr_mi355x: wspr_audio_blanked_batch_device: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_blanked_batch_device/nseg_0_and_bad_pointers 0 |
wspr_audio_blanked_batch_device/no_pcm -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: d_pcm must be 16-byte aligned device memory
wspr_audio_blanked_batch_device/pcm_misaligned -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: d_pcm must be 16-byte aligned device memory
wspr_audio_blanked_batch_device/stride_1004 -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_audio_blanked_batch_device/stride_992 -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_audio_blanked_batch_device/stride_992_and_no_rows -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_audio_blanked_batch_device/no_i -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_audio_blanked_batch_device/no_q -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_audio_blanked_batch_device/i_misaligned -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_audio_blanked_batch_device/thr16_15 -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: thr16 must be 16 .. 4096 and guard 0 .. 64
wspr_audio_blanked_batch_device/guard_65_and_nsamp_1440001 -1 |libwspr_mi355x: wspr_audio_blanked_batch_device: thr16 must be 16 .. 4096 and guard 0 .. 64
wspr_audio_blank_batch_device/fine 0 |
wspr_audio_blank_batch_device/thr16_15 -1 |libwspr_mi355x: wspr_audio_blank_batch_device: thr16 must be 16 .. 4096 and guard 0 .. 64
wspr_audio_blank_batch_device/thr16_4097 -1 |libwspr_mi355x: wspr_audio_blank_batch_device: thr16 must be 16 .. 4096 and guard 0 .. 64
wspr_audio_blank_batch_device/guard_negative -1 |libwspr_mi355x: wspr_audio_blank_batch_device: thr16 must be 16 .. 4096 and guard 0 .. 64
wspr_audio_blank_batch_device/guard_65_and_nsamp_1440001 -1 |libwspr_mi355x: wspr_audio_blank_batch_device: thr16 must be 16 .. 4096 and guard 0 .. 64
wspr_audio_blank_batch_device/nseg_negative_and_no_pcm -1 |libwspr_mi355x: wspr_audio_blank_batch_device: negative count
wspr_audio_blank_batch_device/nsamp_negative -1 |libwspr_mi355x: wspr_audio_blank_batch_device: negative count
wspr_audio_blank_batch_device/nsamp_1440001 -2 |libwspr_mi355x: wspr_audio_blank_batch_device: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_blank_batch_device/nsamp_1440001_and_out_misaligned -2 |libwspr_mi355x: wspr_audio_blank_batch_device: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_blank_batch_device/nseg_0_and_bad_pointers 0 |
wspr_audio_blank_batch_device/no_pcm -1 |libwspr_mi355x: wspr_audio_blank_batch_device: d_pcm must be 16-byte aligned device memory
wspr_audio_blank_batch_device/pcm_misaligned -1 |libwspr_mi355x: wspr_audio_blank_batch_device: d_pcm must be 16-byte aligned device memory
wspr_audio_blank_batch_device/stride_1004 -1 |libwspr_mi355x: wspr_audio_blank_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_audio_blank_batch_device/stride_992_and_no_out -1 |libwspr_mi355x: wspr_audio_blank_batch_device: pcm_stride must be a multiple of 8 and at least nsamp
wspr_audio_blank_batch_device/no_out -1 |libwspr_mi355x: wspr_audio_blank_batch_device: d_out must be 16-byte aligned device memory
wspr_audio_blank_batch_device/out_misaligned -1 |libwspr_mi355x: wspr_audio_blank_batch_device: d_out must be 16-byte aligned device memory
wspr_audio_blank_batch_device/out_stride_1004 -1 |libwspr_mi355x: wspr_audio_blank_batch_device: out_stride must be a multiple of 8 and at least nsamp
wspr_audio_blank_batch_device/out_stride_992 -1 |libwspr_mi355x: wspr_audio_blank_batch_device: out_stride must be a multiple of 8 and at least nsamp
wspr_audio_blank_batch_device/out_stride_992_in_place -1 |libwspr_mi355x: wspr_audio_blank_batch_device: out_stride must be a multiple of 8 and at least nsamp
wspr_audio_blank_batch_device/in_place -1 |libwspr_mi355x: wspr_audio_blank_batch_device: the output rows overlap the input rows
wspr_audio_blank_batch_device/out_begins_in_the_last_input_row -1 |libwspr_mi355x: wspr_audio_blank_batch_device: the output rows overlap the input rows
wspr_audio_blank_batch_device/out_begins_behind_the_last_input_row 0 |
wspr_audio_blank_batch_device/in_place_and_nsamp_0 0 |
wspr_audio_to_iq/fine 0 |
wspr_audio_to_iq/nsamp_1440001_and_no_record -2 |libwspr_mi355x: wspr_audio_to_iq: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_to_iq/no_record -1 |libwspr_mi355x: wspr_audio_to_iq: no record, or no output rows
wspr_audio_to_iq/nsamp_0_and_no_record 0 |
wspr_audio_to_iq/no_i -1 |libwspr_mi355x: wspr_audio_to_iq: no record, or no output rows
wspr_audio_to_iq/nsamp_0_and_no_q -1 |libwspr_mi355x: wspr_audio_to_iq: no record, or no output rows
wspr_audio_to_iq_blanked/fine 0 |
wspr_audio_to_iq_blanked/nsamp_1440001_and_no_record -2 |libwspr_mi355x: wspr_audio_to_iq_blanked: a record holds at most 1440000 samples (120 s); longer ones are refused, not cut
wspr_audio_to_iq_blanked/no_record -1 |libwspr_mi355x: wspr_audio_to_iq_blanked: no record, or no output rows
wspr_audio_to_iq_blanked/nsamp_0_and_no_record 0 |
wspr_audio_to_iq_blanked/no_i -1 |libwspr_mi355x: wspr_audio_to_iq_blanked: no record, or no output rows
wspr_audio_to_iq_blanked/nsamp_0_and_no_q -1 |libwspr_mi355x: wspr_audio_to_iq_blanked: no record, or no output rows
wspr_audio_to_iq_blanked/thr16_15 -1 |libwspr_mi355x: wspr_audio_to_iq_blanked: thr16 must be 16 .. 4096 and guard 0 .. 64
wspr_audio_to_iq_blanked/guard_65_and_nsamp_1440001 -1 |libwspr_mi355x: wspr_audio_to_iq_blanked: thr16 must be 16 .. 4096 and guard 0 .. 64
wspr_noise_batch_device/fine 0 |
wspr_noise_batch_device/default_windows_are_6_42_2672_2790 0 |
wspr_noise_batch_device/whole_row_twice 0 |
wspr_noise_batch_device/the_windows_are_the_callers 0 |
wspr_noise_batch_device/nseg_negative_and_no_rows -1 |libwspr_mi355x: wspr_noise_batch_device: negative count
wspr_noise_batch_device/samples_negative -1 |libwspr_mi355x: wspr_noise_batch_device: negative count
wspr_noise_batch_device/samples_45000 0 |
wspr_noise_batch_device/samples_45001 -2 |libwspr_mi355x: wspr_noise_batch_device: a row holds at most 45000 samples (120 s); longer ones are refused, not cut
wspr_noise_batch_device/samples_45001_and_q_misaligned -2 |libwspr_mi355x: wspr_noise_batch_device: a row holds at most 45000 samples (120 s); longer ones are refused, not cut
wspr_noise_batch_device/samples_45001_and_window_reversed -2 |libwspr_mi355x: wspr_noise_batch_device: a row holds at most 45000 samples (120 s); longer ones are refused, not cut
wspr_noise_batch_device/window_reversed -1 |libwspr_mi355x: wspr_noise_batch_device: a window must satisfy 0 <= b0 <= b1 <= 2812
wspr_noise_batch_device/window_beyond_the_row -1 |libwspr_mi355x: wspr_noise_batch_device: a window must satisfy 0 <= b0 <= b1 <= 2812
wspr_noise_batch_device/window_negative_and_no_out -1 |libwspr_mi355x: wspr_noise_batch_device: a window must satisfy 0 <= b0 <= b1 <= 2812
wspr_noise_batch_device/no_out -1 |libwspr_mi355x: wspr_noise_batch_device: no output records
wspr_noise_batch_device/no_out_and_no_rows -1 |libwspr_mi355x: wspr_noise_batch_device: no output records
wspr_noise_batch_device/nseg_0_and_bad_pointers 0 |
wspr_noise_batch_device/no_i -1 |libwspr_mi355x: wspr_noise_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_noise_batch_device/q_misaligned -1 |libwspr_mi355x: wspr_noise_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_noise_batch_device/q_misaligned_and_stride_odd -1 |libwspr_mi355x: wspr_noise_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_noise_batch_device/stride_1002 -1 |libwspr_mi355x: wspr_noise_batch_device: seg_stride must be a multiple of 4 floats and at least samples
wspr_noise_batch_device/stride_996 -1 |libwspr_mi355x: wspr_noise_batch_device: seg_stride must be a multiple of 4 floats and at least samples
wspr_noise/fine 0 |
wspr_noise/samples_negative -1 |libwspr_mi355x: wspr_noise: negative count
wspr_noise/samples_45001_and_no_row -2 |libwspr_mi355x: wspr_noise: a row holds at most 45000 samples (120 s); longer ones are refused, not cut
wspr_noise/window_reversed -1 |libwspr_mi355x: wspr_noise: a window must satisfy 0 <= b0 <= b1 <= 2812
wspr_noise/no_out_and_no_row -1 |libwspr_mi355x: wspr_noise: no output records
wspr_noise/no_i -1 |libwspr_mi355x: wspr_noise: no row
wspr_noise/no_q -1 |libwspr_mi355x: wspr_noise: no row
wspr_noise/samples_0_and_no_row 0 |
wspr_iq_to_audio_batch_device/fine 0 |
wspr_iq_to_audio_batch_device/nseg_negative_and_no_rows -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: negative count
wspr_iq_to_audio_batch_device/samples_negative -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: negative count
wspr_iq_to_audio_batch_device/samples_45000 0 |
wspr_iq_to_audio_batch_device/samples_45001 -2 |libwspr_mi355x: wspr_iq_to_audio_batch_device: a row holds at most 45000 samples (120 s); longer ones are refused, not cut
wspr_iq_to_audio_batch_device/samples_45001_and_i_misaligned -2 |libwspr_mi355x: wspr_iq_to_audio_batch_device: a row holds at most 45000 samples (120 s); longer ones are refused, not cut
wspr_iq_to_audio_batch_device/samples_45001_and_gain_nan -2 |libwspr_mi355x: wspr_iq_to_audio_batch_device: a row holds at most 45000 samples (120 s); longer ones are refused, not cut
wspr_iq_to_audio_batch_device/gain_nan -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: gain is not finite
wspr_iq_to_audio_batch_device/gain_inf_and_no_rows -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: gain is not finite
wspr_iq_to_audio_batch_device/nseg_0_and_bad_pointers 0 |
wspr_iq_to_audio_batch_device/no_q -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_iq_to_audio_batch_device/i_misaligned_and_stride_odd -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: d_idat and d_qdat must be 16-byte aligned device rows
wspr_iq_to_audio_batch_device/stride_1002 -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: seg_stride must be a multiple of 4 floats and at least samples
wspr_iq_to_audio_batch_device/stride_996_and_no_pcm -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: seg_stride must be a multiple of 4 floats and at least samples
wspr_iq_to_audio_batch_device/no_pcm -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: d_pcm must be 16-byte aligned device memory
wspr_iq_to_audio_batch_device/pcm_misaligned_and_pcm_stride_odd -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: d_pcm must be 16-byte aligned device memory
wspr_iq_to_audio_batch_device/pcm_stride_32004 -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: pcm_stride must be a multiple of 8 and at least 32 * samples
wspr_iq_to_audio_batch_device/pcm_stride_31992 -1 |libwspr_mi355x: wspr_iq_to_audio_batch_device: pcm_stride must be a multiple of 8 and at least 32 * samples
wspr_iq_to_audio/fine 0 |
wspr_iq_to_audio/samples_negative -1 |libwspr_mi355x: wspr_iq_to_audio: negative count
wspr_iq_to_audio/samples_45001_and_no_row -2 |libwspr_mi355x: wspr_iq_to_audio: a row holds at most 45000 samples (120 s); longer ones are refused, not cut
wspr_iq_to_audio/gain_nan_and_no_row -1 |libwspr_mi355x: wspr_iq_to_audio: gain is not finite
wspr_iq_to_audio/no_i -1 |libwspr_mi355x: wspr_iq_to_audio: no row or no output record
wspr_iq_to_audio/no_q -1 |libwspr_mi355x: wspr_iq_to_audio: no row or no output record
wspr_iq_to_audio/no_record -1 |libwspr_mi355x: wspr_iq_to_audio: no row or no output record
wspr_iq_to_audio/samples_0_and_nothing 0 |
"""


def _lines(tmp_path, name, extra):
    exe = os.path.join(str(tmp_path), name)
    subprocess.run(["g++"] + _FLAGS + extra + ["-o", exe, _SRC], check=True)
    r = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert r.stderr == ""
    return r.stdout.rstrip("\n").split("\n")


def _compare(got):
    want = EXPECTED.rstrip("\n").split("\n")
    assert [g.split(" ")[0] for g in got] == [w.split(" ")[0] for w in want], "the table of cases changed"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, "\n".join("got  %s\nwant %s" % gw for gw in wrong)


def test_every_case_answers_as_the_entry_points_did(tmp_path):
    _compare(_lines(tmp_path, "stage_args_check", ["-O2"]))


def test_the_same_under_the_sanitizers(tmp_path):
    _compare(_lines(tmp_path, "stage_args_check_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
