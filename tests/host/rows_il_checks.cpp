// Stand-alone checks of libfpcc_host's interleaved row coder (fpcc_rans_rows_il_encode / _decode of
// fastpcc_amd/csrc/host/rans_host.cpp) for the sanitizer build of tests/test_host_rows_il_sanitized.py: single-threaded, own main,
// linked with the library's source.  Every buffer handed to the library is a heap block of exactly the stated size, so one byte
// outside it is an AddressSanitizer report; UBSan sees the arithmetic.
//
//   rows_il_checks            every check prints `name: ok` or `name: FAIL ...`; exit status 1 if any failed
//   rows_il_checks --list     the names of the checks
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
constexpr int kHeader = 8;

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
    int c = 0;
    std::vector<uint16_t> rows, sym, start, freq_m1;
};

// kind 0: random strictly increasing edges; 1: every symbol but the last has frequency 1 (two-byte emissions); 2: one symbol holds
// 65000 of 65536 (zero-byte emissions)
Case draw(int64_t n, int c, uint64_t seed, int kind) {
    std::mt19937_64 rng(seed);
    Case k;
    k.c = c;
    k.rows.resize(size_t(n) * size_t(c));
    k.sym.resize(size_t(n));
    k.start.resize(size_t(n));
    k.freq_m1.resize(size_t(n));
    std::vector<uint32_t> f(static_cast<size_t>(c));
    for (int64_t i = 0; i < n; ++i) {
        uint32_t s;
        if (kind == 0) {
            uint32_t left = 65536u - uint32_t(c);
            for (int j = 0; j < c; ++j) {
                const uint32_t take = j == c - 1 ? left : uint32_t(rng() % (left / 4 + 1));
                f[size_t(j)] = 1 + take;
                left -= take;
            }
            s = uint32_t(rng() % uint64_t(c));
        } else if (kind == 1) {
            for (int j = 0; j < c; ++j) f[size_t(j)] = 1;
            f[size_t(c - 1)] = 65536u - uint32_t(c - 1);
            s = (rng() % 20 == 0) ? uint32_t(c - 1) : uint32_t(rng() % uint64_t(c - 1));
        } else {
            const uint32_t peak = uint32_t(rng() % uint64_t(c));
            for (int j = 0; j < c; ++j) f[size_t(j)] = 1;
            f[peak] = 65000;
            f[(peak + 1) % uint32_t(c)] += 65536u - 65000u - uint32_t(c - 1);      // what is left goes to one other symbol
            s = (rng() % 32 == 0) ? uint32_t(rng() % uint64_t(c)) : peak;
        }
        uint32_t acc = 0, lo = 0, fr = 0;
        for (int j = 0; j < c; ++j) {
            if (uint32_t(j) == s) { lo = acc; fr = f[size_t(j)]; }
            acc += f[size_t(j)];
            k.rows[size_t(i) * size_t(c) + size_t(j)] = static_cast<uint16_t>(j == c - 1 ? 65535u : acc);
        }
        if (acc != 65536u) { std::fprintf(stderr, "draw: frequencies sum to %u\n", acc); std::abort(); }
        k.sym[size_t(i)] = static_cast<uint16_t>(s);
        k.start[size_t(i)] = static_cast<uint16_t>(lo);
        k.freq_m1[size_t(i)] = static_cast<uint16_t>(fr - 1);
    }
    return k;
}

int64_t worst(int64_t n, int a, int b) {
    const int64_t k = (n + (int64_t(1) << (a + b)) - 1) >> (a + b);
    return kHeader + 4 * k + (int64_t(4) << a) * k + 2 * n;
}

uint64_t seed_of(int64_t n, int c, int a, int b, int kind) { return 100000 * uint64_t(n) + 1000 * uint64_t(c) + 10 * uint64_t(a) + uint64_t(b) + 7 * uint64_t(kind); }

// encode into an exact worst-case block, decode the exact block into an exact output
std::string round_trip(int64_t n, int c, int a, int b, int kind, Bytes *block_out = nullptr) {
    const Case k = draw(n, c, seed_of(n, c, a, b, kind), kind);
    Exact<uint16_t> start(k.start.data(), n), fm1(k.freq_m1.data(), n), rows(k.rows.data(), n * c);
    Exact<uint8_t> out(worst(n, a, b));
    const int64_t len = fpcc_rans_rows_il_encode(start.p, fm1.p, n, c, a, b, out.p, out.n);
    if (len < kHeader) return "encode returned " + std::to_string(len);
    if (kind == 1 && n > 100 && len < 2 * n * 9 / 10) return "two-byte emissions expected";
    Exact<uint8_t> block(out.p, len);
    Exact<uint16_t> got(n);
    const int64_t rc = fpcc_rans_rows_il_decode(block.p, block.n, rows.p, n, c, got.p);
    if (rc != FPCC_HOST_OK) return "decode returned " + std::to_string(rc);
    if (n && std::memcmp(got.p, k.sym.data(), static_cast<size_t>(n) * 2) != 0) return "symbols differ";
    if (len > kHeader) {                             // a block one byte too small for the stream is refused, never overrun
        Exact<uint8_t> tight(len - 1);
        if (fpcc_rans_rows_il_encode(start.p, fm1.p, n, c, a, b, tight.p, tight.n) != FPCC_HOST_E_BUFFER) return "no E_BUFFER one byte short";
    }
    if (block_out) block_out->assign(block.p, block.p + len);
    return "";
}

std::string decode_exact(const Bytes &block, const Case &k, int64_t n, int c, int64_t want, bool either = false) {
    Exact<uint8_t> blk(block.data(), static_cast<int64_t>(block.size()));
    Exact<uint16_t> rows(k.rows.data(), static_cast<int64_t>(k.rows.size()));
    Exact<uint16_t> got(n);
    const int64_t rc = fpcc_rans_rows_il_decode(blk.p, blk.n, rows.p, n, c, got.p);
    if (either && (rc == FPCC_HOST_OK || rc == FPCC_HOST_E_ARG)) return "";
    return rc == want ? "" : "returned " + std::to_string(rc) + ", wanted " + std::to_string(want);
}

void put32(Bytes &b, size_t at, uint32_t v) { for (int i = 0; i < 4; ++i) b[at + i] = static_cast<uint8_t>(v >> (8 * i)); }
uint32_t get32(const Bytes &b, size_t at) { return uint32_t(b[at]) | uint32_t(b[at + 1]) << 8 | uint32_t(b[at + 2]) << 16 | uint32_t(b[at + 3]) << 24; }

struct Check { const char *name; std::function<std::string()> run; };

std::vector<Check> checks() {
    std::vector<Check> out;
    out.push_back({"rows_il_round_trips", [] {
        for (int a : {0, 3, 6})
            for (int b : {4, 6}) {
                const int64_t per = int64_t(1) << (a + b);
                for (int64_t n : {int64_t(0), int64_t(1), int64_t(63), int64_t(64), int64_t(65), per - 1, per, per + 1, 3 * per + 7})
                    for (int c : {2, 255, 256})
                        for (int kind = 0; kind < 3; ++kind) {
                            const std::string e = round_trip(n, c, a, b, kind);
                            if (!e.empty())
                                return "n " + std::to_string(n) + " c " + std::to_string(c) + " a " + std::to_string(a) + " b " + std::to_string(b) +
                                       " kind " + std::to_string(kind) + ": " + e;
                        }
            }
        return std::string();
    }});
    out.push_back({"rows_il_policy_sizes", [] {
        for (int64_t n : {int64_t(0), int64_t(255), int64_t(512), int64_t(5000), int64_t(16383), int64_t(16384), int64_t(70000)}) {
            const int c = 255;
            const Case k = draw(n, c, 5 + uint64_t(n), 2);
            Exact<uint16_t> start(k.start.data(), n), fm1(k.freq_m1.data(), n), rows(k.rows.data(), n * c);
            Exact<uint8_t> outb(worst(n, 6, 10) + 4 * n / 256 + 512);
            const int64_t len = fpcc_rans_rows_il_encode(start.p, fm1.p, n, c, -1, -1, outb.p, outb.n);
            if (len < kHeader || outb.p[1] != 10) return "n " + std::to_string(n) + ": encode " + std::to_string(len);
            const int a = outb.p[0] & 7;
            const int64_t q = n / 256 > 1 ? n / 256 : 1;
            if (n >= 16384 ? a != 6 : !((int64_t(1) << a) <= q && (int64_t(2) << a) > q)) return "n " + std::to_string(n) + ": a = " + std::to_string(a);
            Exact<uint8_t> block(outb.p, len);
            Exact<uint16_t> got(n);
            if (fpcc_rans_rows_il_decode(block.p, block.n, rows.p, n, c, got.p) != FPCC_HOST_OK) return std::string("decode");
            if (n && std::memcmp(got.p, k.sym.data(), static_cast<size_t>(n) * 2) != 0) return std::string("symbols differ");
        }
        return std::string();
    }});
    out.push_back({"rows_il_hostile_headers", [] {
        const int64_t n = 2 * 8 * 16 + 5;
        const int c = 255;
        Bytes block;
        std::string e = round_trip(n, c, 3, 4, 0, &block);
        if (!e.empty()) return e;
        const Case k = draw(n, c, seed_of(n, c, 3, 4, 0), 0);
        const uint32_t l0 = get32(block, 8), l1 = get32(block, 12);
        std::vector<std::pair<const char *, Bytes>> bad;
        { Bytes b = block; b[0] = 0xA3; bad.push_back({"tag", b}); }
        { Bytes b = block; b[0] = 0xB7; bad.push_back({"a = 7", b}); }
        { Bytes b = block; b[0] = 0xBB; bad.push_back({"tag bit 3", b}); }
        { Bytes b = block; b[1] = 3; bad.push_back({"b = 3", b}); }
        { Bytes b = block; b[1] = 13; bad.push_back({"b = 13", b}); }
        { Bytes b = block; b[1] = 255; bad.push_back({"b = 255", b}); }
        { Bytes b = block; put32(b, 2, uint32_t(n) + 1); bad.push_back({"n", b}); }
        { Bytes b = block; put32(b, 2, 0xffffffffu); bad.push_back({"n huge", b}); }
        { Bytes b = block; b[6] = 0; b[7] = 1; bad.push_back({"c = 256", b}); }
        { Bytes b = block; b[6] = 0xff; b[7] = 0xff; bad.push_back({"c huge", b}); }
        { Bytes b = block; put32(b, 8, l0 + 1); bad.push_back({"sum", b}); }
        { Bytes b = block; put32(b, 8, 0xfffffff0u); bad.push_back({"length huge", b}); }
        { Bytes b = block; put32(b, 8, 31); put32(b, 12, l1 + l0 - 31); bad.push_back({"below 4 lanes", b}); }
        { Bytes b = block; b.pop_back(); bad.push_back({"cut by one", b}); }
        { Bytes b(block.begin(), block.begin() + 10); bad.push_back({"no room for lengths", b}); }
        { Bytes b(block.begin(), block.begin() + 8); bad.push_back({"header only", b}); }
        { Bytes b(block.begin(), block.begin() + 7); bad.push_back({"short header", b}); }
        { Bytes b = block; put32(b, kHeader + 12 + 4, 1u << 22); bad.push_back({"state below 2^23", b}); }
        for (auto &kv : bad) {
            e = decode_exact(kv.second, k, n, c, FPCC_HOST_E_ARG);
            if (!e.empty()) return std::string(kv.first) + ": " + e;
        }
        // row widths no decoder takes: refused before a row is read
        for (int bad_c : {1, 0, -5, 257, 70000}) {
            Exact<uint8_t> blk(block.data(), static_cast<int64_t>(block.size()));
            Exact<uint16_t> rows(k.rows.data(), static_cast<int64_t>(k.rows.size()));
            Exact<uint16_t> got(n);
            if (fpcc_rans_rows_il_decode(blk.p, blk.n, rows.p, n, bad_c, got.p) != FPCC_HOST_E_ARG) return "c = " + std::to_string(bad_c) + " accepted";
        }
        // the header of a block for more symbols than the caller has rows for: refused on n, no read of the rows past their end
        Bytes big;
        e = round_trip(5000, c, 6, 4, 0, &big);
        if (!e.empty()) return e;
        return decode_exact(big, k, n, c, FPCC_HOST_E_ARG);
    }});
    out.push_back({"rows_il_hostile_payloads", [] {
        const int64_t n = 2 * 8 * 64 + 500;
        const int c = 255;
        Bytes block;
        std::string e = round_trip(n, c, 3, 6, 1, &block);
        if (!e.empty()) return e;
        const Case k = draw(n, c, seed_of(n, c, 3, 6, 1), 1);
        // the last chunk cut short with a header that still validates: decodes (zeros past the end), stays inside the block, ends
        for (uint32_t drop : {1u, 40u, 400u}) {
            Bytes b = block;
            const uint32_t last = get32(b, kHeader + 8);
            if (last < drop + 32) return std::string("last chunk too small for the test");
            put32(b, kHeader + 8, last - drop);
            b.resize(b.size() - drop);
            e = decode_exact(b, k, n, c, FPCC_HOST_OK);
            if (!e.empty()) return "truncated by " + std::to_string(drop) + ": " + e;
        }
        // random payload bytes behind valid states: any symbols, never a byte outside the block or a row
        std::mt19937_64 rng(99);
        for (int rep = 0; rep < 20; ++rep) {
            Bytes b = block;
            for (size_t i = kHeader + 12 + 32; i < b.size(); ++i) if ((rng() & 3) == 0) b[i] = static_cast<uint8_t>(rng());
            e = decode_exact(b, k, n, c, FPCC_HOST_OK, true);
            if (!e.empty()) return "random payload: " + e;
        }
        // rows that are not CDFs at all (random words, rows that fall): OK or a refusal, never a read outside a row
        Case junk = k;
        for (int rep = 0; rep < 10; ++rep) {
            for (auto &v : junk.rows) v = static_cast<uint16_t>(rep & 1 ? rng() : 65535u - uint32_t(rng() % 300));
            e = decode_exact(block, junk, n, c, FPCC_HOST_OK, true);
            if (!e.empty()) return "junk rows: " + e;
        }
        return std::string();
    }});
    out.push_back({"rows_il_flat_row_refused", [] {
        // symbol 0 is coded with a slot in [100, 200); under the row (300, 50, 50, ..) two entries are <= slot: lo = 50 = hi
        const int64_t n = 300;
        const int c = 4;
        std::vector<uint16_t> start(size_t(n), 300), fm1(size_t(n), 65535 - 300), good, flat;
        start[0] = 100; fm1[0] = 99;
        for (int64_t i = 0; i < n; ++i) {
            for (uint16_t v : {uint16_t(100), uint16_t(200), uint16_t(300), uint16_t(65535)}) good.push_back(v);
            for (uint16_t v : {uint16_t(300), uint16_t(50), uint16_t(50), uint16_t(65535)}) flat.push_back(v);
        }
        Exact<uint16_t> s(start.data(), n), f(fm1.data(), n), g(good.data(), n * c), fl(flat.data(), n * c);
        Exact<uint8_t> outb(worst(n, 3, 4));
        const int64_t len = fpcc_rans_rows_il_encode(s.p, f.p, n, c, 3, 4, outb.p, outb.n);
        if (len < kHeader) return "encode " + std::to_string(len);
        Exact<uint8_t> block(outb.p, len);
        Exact<uint16_t> got(n);
        if (fpcc_rans_rows_il_decode(block.p, block.n, g.p, n, c, got.p) != FPCC_HOST_OK || got.p[0] != 1 || got.p[1] != 3) return std::string("good rows");
        if (fpcc_rans_rows_il_decode(block.p, block.n, fl.p, n, c, got.p) != FPCC_HOST_E_ARG) return std::string("flat row decoded");
        return std::string();
    }});
    out.push_back({"rows_il_encoder_refusals", [] {
        const int64_t n = 300;
        const int c = 255;
        Case k = draw(n, c, 7, 0);
        Exact<uint8_t> outb(worst(n, 3, 4));
        {
            Case bad = k;                            // a range that ends one past the interval
            bad.start[123] = static_cast<uint16_t>(65536u - uint32_t(bad.freq_m1[123]));
            Exact<uint16_t> start(bad.start.data(), n), fm1(bad.freq_m1.data(), n);
            if (bad.start[123] != 0 && fpcc_rans_rows_il_encode(start.p, fm1.p, n, c, 3, 4, outb.p, outb.n) != FPCC_HOST_E_ARG)
                return std::string("a range past 65536 coded");
            bad.start[123] = 65535; bad.freq_m1[123] = 65535;
            Exact<uint16_t> start2(bad.start.data(), n), fm2(bad.freq_m1.data(), n);
            if (fpcc_rans_rows_il_encode(start2.p, fm2.p, n, c, 3, 4, outb.p, outb.n) != FPCC_HOST_E_ARG) return std::string("the widest bad range coded");
        }
        Exact<uint16_t> start(k.start.data(), n), fm1(k.freq_m1.data(), n);
        const int bad_ab[][2] = {{7, 4}, {3, 3}, {3, 13}, {-2, 4}, {64, 4}};
        for (auto &p : bad_ab)
            if (fpcc_rans_rows_il_encode(start.p, fm1.p, n, c, p[0], p[1], outb.p, outb.n) != FPCC_HOST_E_ARG) return std::string("bad a / b accepted");
        for (int bad_c : {1, 0, -1, 257})
            if (fpcc_rans_rows_il_encode(start.p, fm1.p, n, bad_c, 3, 4, outb.p, outb.n) != FPCC_HOST_E_ARG) return std::string("bad c accepted");
        if (fpcc_rans_rows_il_encode(start.p, fm1.p, n, c, 3, 4, outb.p, 7) != FPCC_HOST_E_BUFFER) return std::string("no room for a header");
        if (fpcc_rans_rows_il_encode(start.p, fm1.p, -1, c, 3, 4, outb.p, outb.n) != FPCC_HOST_E_ARG) return std::string("negative n");
        if (fpcc_rans_rows_il_encode(start.p, fm1.p, n, c, 3, 4, nullptr, outb.n) != FPCC_HOST_E_ARG) return std::string("null out");
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
