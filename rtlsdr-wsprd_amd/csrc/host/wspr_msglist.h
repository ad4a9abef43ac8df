// The message list of the list-decoding stage (wspr_set_message_list(); the definition in kernels/listmatch.h): what an
// entry is, the process-wide list and the snapshot a decode call takes of it.  Pure host C++.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

namespace wspr {

// One list, immutable once built.  A call holds it through a shared_ptr, so a setter that runs meanwhile replaces the
// process-wide list without touching what the call works on.
struct MessageList {
    uint64_t generation = 0;                        // unique per successful wspr_set_message_list() of this process, never 0
    int zmin16 = 0;
    int n = 0;                                      // entries kept
    std::vector<char> text;                         // [n][23] canonical texts
    std::vector<unsigned char> decdata;             // [n][11] as the Fano decoder leaves them
    std::vector<unsigned char> symbols;             // [n][162] channel symbols 0..3
    std::vector<int32_t> table;                     // [48][padded(n)] words of four int8 chips (listmatch.h: the device layout)
    std::vector<int32_t> bias;                      // [padded(n)] B_m
};

// Builds a list from n texts.  Null with `bad` = the first offending index when a text does not qualify (bad = -1: n or
// zmin16 out of range).  Entries whose 50 bits repeat an earlier entry are dropped.
std::shared_ptr<const MessageList> build_message_list(const char* const* messages, int n, int zmin16, int* bad);

// The process-wide list (null: the stage is off) ...
std::shared_ptr<const MessageList> message_list_setting();
void set_message_list_setting(std::shared_ptr<const MessageList> list);
// ... of which a decode call takes a snapshot on entry, with its other settings (CallSettings in wspr_pipeline.h)

}  // namespace wspr
