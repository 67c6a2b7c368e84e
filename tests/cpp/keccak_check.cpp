// Host check of mxx_amd/csrc/keccak.h (tests/test_keccak_host.py builds it with -fsanitize=address,undefined).
// stdin: one message per line, "<padding byte, two hex digits> <message in hex, or - for the empty message>";
// stdout: the 32-byte digest in hex, one line per message.
#include "../../mxx_amd/csrc/keccak.h"

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

static int nibble(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const size_t gap = line.find(' ');
        if (gap != 2 || nibble(line[0]) < 0 || nibble(line[1]) < 0) {
            std::fprintf(stderr, "keccak_check: malformed line\n");
            return 2;
        }
        const uint8_t pad = static_cast<uint8_t>(nibble(line[0]) * 16 + nibble(line[1]));
        const std::string hex = line.substr(gap + 1) == "-" ? std::string() : line.substr(gap + 1);
        if (hex.size() % 2) {
            std::fprintf(stderr, "keccak_check: odd number of hex digits\n");
            return 2;
        }
        // exactly the message's bytes on the heap: a read past them is the sanitizer's to report
        std::vector<uint8_t> msg(hex.size() / 2);
        for (size_t i = 0; i < msg.size(); ++i) {
            const int hi = nibble(hex[2 * i]), lo = nibble(hex[2 * i + 1]);
            if (hi < 0 || lo < 0) {
                std::fprintf(stderr, "keccak_check: not a hex digit\n");
                return 2;
            }
            msg[i] = static_cast<uint8_t>(hi * 16 + lo);
        }
        const uint8_t *bytes = msg.data();
        uint64_t digest[4];
        keccak_sponge256([bytes](size_t pos) { return bytes[pos]; }, msg.size(), pad, digest);
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 8; ++k) std::printf("%02x", static_cast<unsigned>((digest[i] >> (8 * k)) & 0xFF));
        std::printf("\n");
    }
    return 0;
}
