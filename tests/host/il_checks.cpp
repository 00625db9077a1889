// Stand-alone checks of libfpcc_host's interleaved binary coder (fpcc_rans_binary_il_encode / _decode of
// fastpcc_amd/csrc/host/rans_host.cpp) for the sanitizer build of tests/test_host_il_sanitized.py: single-threaded, own main, linked
// with the library's source.  Every buffer handed to the library is a heap block of exactly the stated size, so one byte outside it
// is an AddressSanitizer report; UBSan sees the arithmetic.
//
//   il_checks            every check prints `name: ok` or `name: FAIL ...`; exit status 1 if any failed
//   il_checks --list     the names of the checks
#include "../../include/fpcc_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

namespace {

using Bytes = std::vector<uint8_t>;

template <class T>
struct Exact {                                       // a heap block of exactly `n` elements
    T *p;
    int64_t n;
    explicit Exact(int64_t count) : p(static_cast<T *>(std::malloc(static_cast<size_t>(count ? count : 1) * sizeof(T)))), n(count) {
        if (!count) { std::free(p); p = static_cast<T *>(std::malloc(0)); }
    }
    Exact(const T *src, int64_t count) : Exact(count) { if (n) std::memcpy(p, src, static_cast<size_t>(n) * sizeof(T)); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
    ~Exact() { std::free(p); }
};

struct Case {
    std::vector<uint8_t> bits;
    std::vector<uint16_t> prob;
};

Case draw(int64_t n, uint64_t seed, int kind) {
    std::mt19937_64 rng(seed);
    Case c;
    c.bits.resize(static_cast<size_t>(n));
    c.prob.resize(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) {
        uint32_t p;
        if (kind == 0) {                             // mass near both ends, as an occupancy predictor's
            const double u = double(rng() >> 11) / double(1ull << 53);
            const double v = u < 0.5 ? u * u * 2 : 1 - (1 - u) * (1 - u) * 2;
            p = static_cast<uint32_t>(v * 65536.0);
        } else {                                     // the least likely symbol every time: two bytes per symbol
            p = (rng() & 1) ? 1u : 65535u;
        }
        p = p < 1 ? 1 : (p > 65535 ? 65535 : p);
        c.prob[size_t(i)] = static_cast<uint16_t>(p);
        c.bits[size_t(i)] = kind == 0 ? static_cast<uint8_t>((rng() & 0xffff) < p) : static_cast<uint8_t>(p == 1);
    }
    return c;
}

int64_t worst(int64_t n, int a, int b) {
    const int64_t k = (n + (int64_t(1) << (a + b)) - 1) >> (a + b);
    return 6 + 4 * k + (int64_t(4) << a) * k + 2 * n;
}

// encode into an exact worst-case block, decode the exact block into an exact output
std::string round_trip(int64_t n, int a, int b, int kind, Bytes *block_out = nullptr) {
    const Case c = draw(n, 1000 * uint64_t(n) + 10 * a + b + kind, kind);
    Exact<uint8_t> bits(c.bits.data(), n);
    Exact<uint16_t> prob(c.prob.data(), n);
    Exact<uint8_t> out(worst(n, a, b));
    const int64_t len = fpcc_rans_binary_il_encode(bits.p, prob.p, n, a, b, out.p, out.n);
    if (len < 6) return "encode returned " + std::to_string(len);
    if (kind == 1 && n > 0 && len < 2 * n) return "two-byte emissions expected";
    Exact<uint8_t> block(out.p, len);
    Exact<uint8_t> got(n);
    const int64_t rc = fpcc_rans_binary_il_decode(block.p, block.n, prob.p, n, got.p);
    if (rc != FPCC_HOST_OK) return "decode returned " + std::to_string(rc);
    if (n && std::memcmp(got.p, bits.p, static_cast<size_t>(n)) != 0) return "bits differ";
    // a block one byte too small for the stream is refused, never overrun
    if (len > 6) {
        Exact<uint8_t> tight(len - 1);
        if (fpcc_rans_binary_il_encode(bits.p, prob.p, n, a, b, tight.p, tight.n) != FPCC_HOST_E_BUFFER) return "no E_BUFFER one byte short";
    }
    if (block_out) block_out->assign(block.p, block.p + len);
    return "";
}

std::string decode_exact(const Bytes &block, const std::vector<uint16_t> &prob, int64_t want) {
    Exact<uint8_t> blk(block.data(), static_cast<int64_t>(block.size()));
    Exact<uint16_t> p(prob.data(), static_cast<int64_t>(prob.size()));
    Exact<uint8_t> got(static_cast<int64_t>(prob.size()));
    const int64_t rc = fpcc_rans_binary_il_decode(blk.p, blk.n, p.p, p.n, got.p);
    return rc == want ? "" : "returned " + std::to_string(rc) + ", wanted " + std::to_string(want);
}

void put32(Bytes &b, size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) b[at + i] = static_cast<uint8_t>(v >> (8 * i)); }
uint32_t get32(const Bytes &b, size_t at) { return uint32_t(b[at]) | uint32_t(b[at + 1]) << 8 | uint32_t(b[at + 2]) << 16 | uint32_t(b[at + 3]) << 24; }

struct Check { const char *name; std::function<std::string()> run; };

std::vector<Check> checks() {
    std::vector<Check> out;
    out.push_back({"il_round_trips", [] {
        const int ab[][2] = {{0, 4}, {3, 4}, {6, 4}, {6, 6}};
        const int64_t sizes[] = {0, 1, 63, 64, 65, 1000, 2 * 64 * 16 + 5, 2 * 64 * 64 + 5};
        for (auto &p : ab)
            for (int64_t n : sizes)
                for (int kind = 0; kind < 2; ++kind) {
                    const std::string e = round_trip(n, p[0], p[1], kind);
                    if (!e.empty()) return "n " + std::to_string(n) + " a " + std::to_string(p[0]) + " b " + std::to_string(p[1]) + ": " + e;
                }
        return std::string();
    }});
    out.push_back({"il_policy_sizes", [] {
        for (int64_t n : {int64_t(0), int64_t(255), int64_t(512), int64_t(5000), int64_t(16383), int64_t(16384), int64_t(70000)}) {
            const Case c = draw(n, 5 + uint64_t(n), 0);
            Exact<uint8_t> bits(c.bits.data(), n);
            Exact<uint16_t> prob(c.prob.data(), n);
            Exact<uint8_t> out(worst(n, 6, 10) + 4 * n / 256 + 512);
            const int64_t len = fpcc_rans_binary_il_encode(bits.p, prob.p, n, -1, -1, out.p, out.n);
            if (len < 6 || out.p[1] != 10) return "n " + std::to_string(n) + ": encode " + std::to_string(len);
            const int a = out.p[0] & 7;
            const int64_t q = n / 256 > 1 ? n / 256 : 1;
            if (n >= 16384 ? a != 6 : !((int64_t(1) << a) <= q && (int64_t(2) << a) > q)) return "n " + std::to_string(n) + ": a = " + std::to_string(a);
            Exact<uint8_t> block(out.p, len);
            Exact<uint8_t> got(n);
            if (fpcc_rans_binary_il_decode(block.p, block.n, prob.p, n, got.p) != FPCC_HOST_OK) return std::string("decode");
            if (n && std::memcmp(got.p, bits.p, static_cast<size_t>(n)) != 0) return std::string("bits differ");
        }
        return std::string();
    }});
    out.push_back({"il_hostile_headers", [] {
        const int64_t n = 2 * 8 * 16 + 5;
        Bytes block;
        std::string e = round_trip(n, 3, 4, 0, &block);
        if (!e.empty()) return e;
        const Case c = draw(n, 1000 * uint64_t(n) + 10 * 3 + 4, 0);
        const uint32_t l0 = get32(block, 6), l1 = get32(block, 10);
        std::vector<std::pair<const char *, Bytes>> bad;
        { Bytes b = block; b[0] = 0x53; bad.push_back({"tag", b}); }
        { Bytes b = block; b[0] = 0xA7; bad.push_back({"a = 7", b}); }
        { Bytes b = block; b[0] = 0xAB; bad.push_back({"tag bit 3", b}); }
        { Bytes b = block; b[1] = 3; bad.push_back({"b = 3", b}); }
        { Bytes b = block; b[1] = 13; bad.push_back({"b = 13", b}); }
        { Bytes b = block; b[1] = 255; bad.push_back({"b = 255", b}); }
        { Bytes b = block; put32(b, 2, uint32_t(n) + 1); bad.push_back({"n", b}); }
        { Bytes b = block; put32(b, 2, 0xffffffffu); bad.push_back({"n huge", b}); }
        { Bytes b = block; put32(b, 6, l0 + 1); bad.push_back({"sum", b}); }
        { Bytes b = block; put32(b, 6, 0xfffffff0u); bad.push_back({"length huge", b}); }
        { Bytes b = block; put32(b, 6, 31); put32(b, 10, l1 + l0 - 31); bad.push_back({"below 4 lanes", b}); }
        { Bytes b = block; b.pop_back(); bad.push_back({"cut by one", b}); }
        { Bytes b(block.begin(), block.begin() + 8); bad.push_back({"no room for lengths", b}); }
        { Bytes b(block.begin(), block.begin() + 6); bad.push_back({"header only", b}); }
        { Bytes b(block.begin(), block.begin() + 5); bad.push_back({"short header", b}); }
        { Bytes b = block; put32(b, 6 + 12 + 4, 1u << 22); bad.push_back({"state below 2^23", b}); }
        for (auto &kv : bad) {
            e = decode_exact(kv.second, c.prob, FPCC_HOST_E_ARG);
            if (!e.empty()) return std::string(kv.first) + ": " + e;
        }
        // the header of a block for more symbols than the caller has probabilities for: refused on n, no read of prob1 past its end
        Bytes big;
        e = round_trip(70000, 6, 4, 0, &big);
        if (!e.empty()) return e;
        return decode_exact(big, c.prob, FPCC_HOST_E_ARG);
    }});
    out.push_back({"il_hostile_payloads", [] {
        const int64_t n = 2 * 8 * 64 + 500;
        Bytes block;
        std::string e = round_trip(n, 3, 6, 1, &block);
        if (!e.empty()) return e;
        const Case c = draw(n, 1000 * uint64_t(n) + 10 * 3 + 6 + 1, 1);
        // the last chunk cut short with a header that still validates: decodes (zeros past the end), stays inside the block, ends
        for (uint32_t drop : {1u, 40u, 400u}) {
            Bytes b = block;
            const uint32_t last = get32(b, 6 + 8);
            if (last < drop + 32) return std::string("last chunk too small for the test");
            put32(b, 6 + 8, last - drop);
            b.resize(b.size() - drop);
            e = decode_exact(b, c.prob, FPCC_HOST_OK);
            if (!e.empty()) return "truncated by " + std::to_string(drop) + ": " + e;
        }
        // random payload bytes behind valid states: any bits, never a byte outside the block
        std::mt19937_64 rng(99);
        for (int rep = 0; rep < 20; ++rep) {
            Bytes b = block;
            for (size_t i = 6 + 12 + 32; i < b.size(); ++i) if ((rng() & 3) == 0) b[i] = static_cast<uint8_t>(rng());
            Exact<uint8_t> blk(b.data(), static_cast<int64_t>(b.size()));
            Exact<uint16_t> p(c.prob.data(), n);
            Exact<uint8_t> got(n);
            const int64_t rc = fpcc_rans_binary_il_decode(blk.p, blk.n, p.p, n, got.p);
            if (rc != FPCC_HOST_OK && rc != FPCC_HOST_E_ARG) return "random payload: " + std::to_string(rc);
        }
        return std::string();
    }});
    out.push_back({"il_encoder_refusals", [] {
        const int64_t n = 300;
        Case c = draw(n, 7, 0);
        c.prob[123] = 0;
        for (int bit = 0; bit < 2; ++bit) {
            c.bits[123] = static_cast<uint8_t>(bit);
            Exact<uint8_t> bits(c.bits.data(), n);
            Exact<uint16_t> prob(c.prob.data(), n);
            Exact<uint8_t> out(worst(n, 3, 4));
            if (fpcc_rans_binary_il_encode(bits.p, prob.p, n, 3, 4, out.p, out.n) != FPCC_HOST_E_ARG) return std::string("zero probability coded");
        }
        c.prob[123] = 7;
        Exact<uint8_t> bits(c.bits.data(), n);
        Exact<uint16_t> prob(c.prob.data(), n);
        Exact<uint8_t> out(worst(n, 3, 4));
        const int bad_ab[][2] = {{7, 4}, {3, 3}, {3, 13}, {-2, 4}, {64, 4}};
        for (auto &p : bad_ab)
            if (fpcc_rans_binary_il_encode(bits.p, prob.p, n, p[0], p[1], out.p, out.n) != FPCC_HOST_E_ARG) return std::string("bad a / b accepted");
        if (fpcc_rans_binary_il_encode(bits.p, prob.p, n, 3, 4, out.p, 5) != FPCC_HOST_E_BUFFER) return std::string("no room for a header");
        if (fpcc_rans_binary_il_encode(bits.p, prob.p, -1, 3, 4, out.p, out.n) != FPCC_HOST_E_ARG) return std::string("negative n");
        if (fpcc_rans_binary_il_encode(bits.p, prob.p, n, 3, 4, nullptr, out.n) != FPCC_HOST_E_ARG) return std::string("null out");
        return std::string();
    }});
    return out;
}

}  // namespace

int main(int argc, char **argv) {
    const auto all = checks();
    if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
        for (auto &c : all) std::printf("%s\n", c.name);
        return 0;
    }
    int failed = 0;
    for (auto &c : all) {
        const std::string e = c.run();
        if (e.empty()) std::printf("%s: ok\n", c.name);
        else { std::printf("%s: FAIL %s\n", c.name, e.c_str()); ++failed; }
        std::fflush(stdout);
    }
    return failed ? 1 : 0;
}
