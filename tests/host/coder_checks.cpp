// Stand-alone checks of libfpcc_host's coders (fastpcc_amd/csrc/host/rans_host.cpp) for the sanitizer builds of
// tests/test_host_sanitized.py: single-threaded, own main, linked with the library's source and with the plain-C test oracle
// oracle/rans.c.  Every buffer handed to the library is a heap block of exactly the stated size, so one byte outside it is an
// AddressSanitizer report; UBSan sees the arithmetic.
//
//   coder_checks GOLDEN_FLAT_FILE [--only SUBSTRING]     every check prints `name: ok` or `name: FAIL ...`; exit status 1 if any failed
//   coder_checks --list                                  the names of the checks
//   coder_checks --time                                  ns per symbol of fpcc_rans_binary_encode and fpcc_simple_enc_push_ranges
//
// GOLDEN_FLAT_FILE is written by the Python test from tests/golden/rans.json and rans_random.json: whitespace-separated tokens, one
// record per case (`cdf`, `indexed`, `binary`, `simple`, `simplebin`, `random`), numbers in decimal, doubles as C hex floats,
// streams as hex strings.
#include "../../include/fpcc_host.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdarg>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <vector>

extern "C" {
int64_t orc_pmf_to_cdf(double *pmf, int64_t n, int overflow_mode, int32_t *offset, uint32_t *cdf_out);
int64_t orc_indexed_encode(const int32_t *sym, const int32_t *index, int64_t n, const uint32_t *cdfs, const int64_t *cdf_start,
                           const int64_t *cdf_len, const int32_t *offsets, int64_t n_tables, int escape_mode, uint8_t *out, int64_t cap);
void orc_indexed_decode(const uint8_t *bytes, const int32_t *index, int64_t n, const uint32_t *cdfs, const int64_t *cdf_start,
                        const int64_t *cdf_len, const int32_t *offsets, int64_t n_tables, int escape_mode, int32_t *sym_out);
int64_t orc_binary_encode(const uint8_t *bits, const uint32_t *prob1, int64_t n, uint8_t *out, int64_t cap);
void orc_binary_decode(const uint8_t *bytes, const uint32_t *prob1, int64_t n, uint8_t *bits_out);
struct orc_simple_enc;
struct orc_simple_dec;
orc_simple_enc *orc_simple_enc_new(int64_t cap);
void orc_simple_enc_free(orc_simple_enc *s);
int64_t orc_simple_enc_push(orc_simple_enc *s, const uint16_t *rows, int64_t n_rows, int64_t width, const uint16_t *sym, int64_t n);
int64_t orc_simple_enc_push_bin(orc_simple_enc *s, const uint16_t *edge, int64_t n_rows, const uint8_t *bits, int64_t n);
int64_t orc_simple_enc_finish(orc_simple_enc *s, uint8_t *out, int64_t out_cap);
orc_simple_dec *orc_simple_dec_new(const uint8_t *bytes);
void orc_simple_dec_free(orc_simple_dec *s);
void orc_simple_dec_pop(orc_simple_dec *s, const uint16_t *rows, int64_t n_rows, int64_t width, uint16_t *sym_out, int64_t n);
void orc_simple_dec_pop_bin(orc_simple_dec *s, const uint16_t *edge, int64_t n_rows, uint8_t *bits_out, int64_t n);
}

namespace {

using Bytes = std::vector<uint8_t>;
using Rng = std::mt19937_64;
constexpr int64_t OK = FPCC_HOST_OK, E_BUFFER = FPCC_HOST_E_BUFFER, E_ARG = FPCC_HOST_E_ARG, E_CDF = FPCC_HOST_E_CDF;

// a heap block of exactly `n` elements
template <class T>
struct Exact {
    T *p;
    int64_t n;
    explicit Exact(int64_t count) : p(static_cast<T *>(std::malloc(static_cast<size_t>(count) * sizeof(T)))), n(count) {}
    explicit Exact(const std::vector<T> &v) : Exact(static_cast<int64_t>(v.size())) {
        if (n) std::memcpy(p, v.data(), static_cast<size_t>(n) * sizeof(T));
    }
    Exact(const T *src, int64_t count) : Exact(count) { if (n) std::memcpy(p, src, static_cast<size_t>(n) * sizeof(T)); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
    ~Exact() { std::free(p); }
    std::vector<T> vec() const { return std::vector<T>(p, p + n); }
};

std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char *f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

#define REQUIRE(cond, ...) do { if (!(cond)) return std::string(#cond) + ": " + fmt(__VA_ARGS__); } while (0)
#define EXPECT_RC(expr, want, ...) do { const int64_t rc_ = (expr); if (rc_ != (want)) \
    return std::string(#expr) + fmt(" returned %lld, expected %lld: ", (long long)rc_, (long long)(want)) + fmt(__VA_ARGS__); } while (0)
#define PROPAGATE(expr) do { const std::string m_ = (expr); if (!m_.empty()) return m_; } while (0)

// ---- tables of the indexed coder ------------------------------------------------------------------------------------------------
struct Tab {
    std::vector<uint32_t> flat;
    std::vector<int64_t> start, len;
    std::vector<int32_t> off;
    int64_t count() const { return static_cast<int64_t>(len.size()); }
};

Tab make_tab(const std::vector<std::vector<uint32_t>> &rows, const std::vector<int32_t> &off) {
    Tab t;
    for (const auto &r : rows) {
        t.start.push_back(static_cast<int64_t>(t.flat.size()));
        t.len.push_back(static_cast<int64_t>(r.size()));
        t.flat.insert(t.flat.end(), r.begin(), r.end());
    }
    t.off = off;
    return t;
}

// a strictly increasing quantised CDF with `bins` bins
std::vector<uint32_t> rand_cdf(Rng &rng, int bins) {
    std::vector<uint32_t> cuts;
    while (static_cast<int>(cuts.size()) < bins - 1) {
        for (int k = static_cast<int>(cuts.size()); k < bins - 1; ++k) cuts.push_back(1 + static_cast<uint32_t>(rng() % 65535));
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    }
    std::vector<uint32_t> c{0};
    c.insert(c.end(), cuts.begin(), cuts.end());
    c.push_back(65536);
    return c;
}

// the library's indexed coder on exact heap copies of every operand; the stream is returned without the unused head of `out`
int64_t lib_idx_enc(const Tab &t, const std::vector<int32_t> &sym, const std::vector<int32_t> *index, int overflow, int64_t cap, Bytes &stream) {
    Exact<int32_t> s(sym), o(t.off);
    Exact<int32_t> ix(index ? *index : std::vector<int32_t>());
    Exact<uint32_t> c(t.flat);
    Exact<int64_t> st(t.start), ln(t.len);
    Exact<uint8_t> out(cap);
    const int64_t rc = fpcc_rans_indexed_encode(s.p, index ? ix.p : nullptr, s.n, c.p, st.p, ln.p, o.p, t.count(), overflow, out.p, cap);
    if (rc >= 0 && rc <= cap) stream.assign(out.p + cap - rc, out.p + cap);
    return rc;
}

int64_t lib_idx_dec(const Tab &t, const Bytes &stream, const std::vector<int32_t> *index, int64_t n, int overflow, std::vector<int32_t> &sym) {
    Exact<uint8_t> b(stream);
    Exact<int32_t> o(t.off), out(n);
    Exact<int32_t> ix(index ? *index : std::vector<int32_t>());
    Exact<uint32_t> c(t.flat);
    Exact<int64_t> st(t.start), ln(t.len);
    for (int64_t i = 0; i < n; ++i) out.p[i] = 0x5a5a5a5a;
    const int64_t rc = fpcc_rans_indexed_decode(b.p, b.n, index ? ix.p : nullptr, n, c.p, st.p, ln.p, o.p, t.count(), overflow, out.p);
    sym = out.vec();
    return rc;
}

Bytes orc_idx_enc(const Tab &t, const std::vector<int32_t> &sym, const std::vector<int32_t> *index, int overflow) {
    const int64_t n = static_cast<int64_t>(sym.size()), cap = 40 * n + 64;
    Bytes out(static_cast<size_t>(cap));
    const int64_t got = orc_indexed_encode(sym.data(), index ? index->data() : nullptr, n, t.flat.data(), t.start.data(), t.len.data(),
                                           t.off.data(), t.count(), overflow, out.data(), cap);
    if (got < 0) return Bytes();
    return Bytes(out.end() - got, out.end());
}

// library == oracle bytes, both decoders give the symbols back
std::string idx_differential(const Tab &t, const std::vector<int32_t> &sym, const std::vector<int32_t> *index, int overflow, const char *what) {
    const int64_t n = static_cast<int64_t>(sym.size());
    Bytes got;
    EXPECT_RC(lib_idx_enc(t, sym, index, overflow, 40 * n + 64, got) < 0 ? -1 : 0, 0, "%s: encode", what);
    const Bytes want = orc_idx_enc(t, sym, index, overflow);
    REQUIRE(got == want, "%s: %zu library bytes, %zu oracle bytes", what, got.size(), want.size());
    std::vector<int32_t> back;
    EXPECT_RC(lib_idx_dec(t, got, index, n, overflow, back), OK, "%s: decode", what);
    REQUIRE(back == sym, "%s: library decode differs", what);
    std::vector<int32_t> oback(static_cast<size_t>(n));
    orc_indexed_decode(got.data(), index ? index->data() : nullptr, n, t.flat.data(), t.start.data(), t.len.data(), t.off.data(), t.count(),
                       overflow, oback.data());
    REQUIRE(oback == sym, "%s: oracle decode of the library's stream differs", what);
    return "";
}

// ---- binary coder ---------------------------------------------------------------------------------------------------------------
int64_t lib_bin_enc(const std::vector<uint8_t> &bits, const std::vector<uint16_t> &prob, int64_t cap, Bytes &stream) {
    Exact<uint8_t> b(bits), out(cap);
    Exact<uint16_t> p(prob);
    const int64_t rc = fpcc_rans_binary_encode(b.p, p.p, b.n, out.p, cap);
    if (rc >= 0 && rc <= cap) stream.assign(out.p + cap - rc, out.p + cap);
    return rc;
}

int64_t lib_bin_dec(const Bytes &stream, const std::vector<uint16_t> &prob, std::vector<uint8_t> &bits) {
    Exact<uint8_t> s(stream), out(static_cast<int64_t>(prob.size()));
    Exact<uint16_t> p(prob);
    if (out.n) std::memset(out.p, 0x5a, static_cast<size_t>(out.n));
    const int64_t rc = fpcc_rans_binary_decode(s.p, s.n, p.p, p.n, out.p);
    bits = out.vec();
    return rc;
}

Bytes orc_bin_enc(const std::vector<uint8_t> &bits, const std::vector<uint16_t> &prob) {
    const int64_t n = static_cast<int64_t>(bits.size()), cap = 2 * n + 64;
    std::vector<uint32_t> p32(prob.begin(), prob.end());
    Bytes out(static_cast<size_t>(cap));
    const int64_t got = orc_binary_encode(bits.data(), p32.data(), n, out.data(), cap);
    if (got < 0) return Bytes();
    return Bytes(out.end() - got, out.end());
}

void rand_binary(Rng &rng, int64_t n, std::vector<uint8_t> &bits, std::vector<uint16_t> &prob) {
    static const uint16_t kEdge[5] = {1, 2, 32768, 65534, 65535};
    bits.resize(static_cast<size_t>(n));
    prob.resize(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) {
        prob[i] = rng() % 3 == 0 ? kEdge[rng() % 5] : static_cast<uint16_t>(1 + rng() % 65535);
        // mostly drawn from the model, sometimes against it (the improbable symbol of an extreme probability is the long code)
        bits[i] = rng() % 8 == 0 ? static_cast<uint8_t>(rng() & 1) : static_cast<uint8_t>((rng() & 0xffff) < prob[i]);
    }
}

// ---- persistent coder -----------------------------------------------------------------------------------------------------------
// one block of a persistent stream
struct Block {
    enum Kind { ROWS, BIN, RANGES } kind = ROWS;
    int64_t n_rows = 0, width = 0, n = 0;
    std::vector<uint16_t> rows;      // ROWS, RANGES: [n_rows, width]; BIN: edge[n_rows]
    std::vector<uint16_t> sym;       // ROWS, RANGES
    std::vector<uint8_t> bits;       // BIN
};

void row_range(const uint16_t *row, int64_t width, uint32_t s, uint32_t &lo, uint32_t &hi) {
    lo = s ? row[s - 1] : 0u;
    hi = static_cast<int64_t>(s) == width - 1 ? 65536u : row[s];
}

int64_t lib_push(fpcc_simple_enc *e, const Block &b) {
    if (b.kind == Block::BIN) {
        Exact<uint16_t> edge(b.rows);
        Exact<uint8_t> bits(b.bits);
        return fpcc_simple_enc_push_bin(e, edge.p, b.n_rows, bits.p, b.n);
    }
    if (b.kind == Block::RANGES) {
        std::vector<uint16_t> start(static_cast<size_t>(b.n)), fm1(static_cast<size_t>(b.n));
        for (int64_t i = 0; i < b.n; ++i) {
            uint32_t lo, hi;
            row_range(b.rows.data() + (b.n_rows == 1 ? 0 : i * b.width), b.width, b.sym[i], lo, hi);
            start[i] = static_cast<uint16_t>(lo);
            fm1[i] = static_cast<uint16_t>(hi - lo - 1);
        }
        Exact<uint16_t> s(start), f(fm1);
        return fpcc_simple_enc_push_ranges(e, s.p, f.p, b.n);
    }
    Exact<uint16_t> rows(b.rows), sym(b.sym);
    return fpcc_simple_enc_push(e, rows.p, b.n_rows, b.width, sym.p, b.n);
}

int64_t lib_finish(fpcc_simple_enc *e, int64_t cap, Bytes &stream) {
    Exact<uint8_t> out(cap);
    const int64_t rc = fpcc_simple_enc_finish(e, out.p, cap);
    if (rc >= 0 && rc <= cap) stream.assign(out.p, out.p + rc);
    return rc;
}

Bytes orc_simple_stream(const std::vector<Block> &blocks, int64_t cap) {
    orc_simple_enc *e = orc_simple_enc_new(cap);
    for (const Block &b : blocks) {
        if (b.kind == Block::BIN) orc_simple_enc_push_bin(e, b.rows.data(), b.n_rows, b.bits.data(), b.n);
        else orc_simple_enc_push(e, b.rows.data(), b.n_rows, b.width, b.sym.data(), b.n);          // RANGES: the rows define the stream
    }
    Bytes out(static_cast<size_t>(cap));
    const int64_t got = orc_simple_enc_finish(e, out.data(), cap);
    orc_simple_enc_free(e);
    out.resize(got < 0 ? 0 : static_cast<size_t>(got));
    return out;
}

// the oracle decoder's read position: orc_simple_dec starts with oracle/rans.c's `struct { const uint8_t *p; uint32_t x; }`
struct OrcDecView { const uint8_t *p; uint32_t x; };

// library stream == oracle stream; blocks popped in reverse give the symbols back, and after each block the library's decoder stands
// where the oracle's does
std::string simple_differential(const std::vector<Block> &blocks, const char *what) {
    const int64_t cap = 1 << 20;
    fpcc_simple_enc *e = fpcc_simple_enc_new(cap);
    REQUIRE(e != nullptr, "%s: no encoder", what);
    for (size_t k = 0; k < blocks.size(); ++k) {
        const int64_t rc = lib_push(e, blocks[k]);
        if (rc < 0) { fpcc_simple_enc_free(e); return fmt("%s: push of block %zu returned %lld", what, k, (long long)rc); }
    }
    Bytes got;
    const int64_t len = lib_finish(e, cap, got);
    fpcc_simple_enc_free(e);
    REQUIRE(len >= 4, "%s: finish returned %lld", what, (long long)len);
    const Bytes want = orc_simple_stream(blocks, cap);
    REQUIRE(got == want, "%s: %zu library bytes, %zu oracle bytes", what, got.size(), want.size());
    Exact<uint8_t> stream(got);
    fpcc_simple_dec *d = fpcc_simple_dec_new(stream.p, stream.n);
    REQUIRE(d != nullptr, "%s: no decoder", what);
    orc_simple_dec *od = orc_simple_dec_new(got.data());
    std::string msg;
    for (size_t k = blocks.size(); k-- > 0 && msg.empty();) {
        const Block &b = blocks[k];
        if (b.kind == Block::BIN) {
            Exact<uint16_t> edge(b.rows);
            Exact<uint8_t> out(b.n);
            std::vector<uint8_t> oout(static_cast<size_t>(b.n));
            const int64_t rc = fpcc_simple_dec_pop_bin(d, edge.p, b.n_rows, out.p, b.n);
            orc_simple_dec_pop_bin(od, b.rows.data(), b.n_rows, oout.data(), b.n);
            if (rc != OK || out.vec() != b.bits || oout != b.bits) msg = fmt("%s: block %zu (bin) decodes wrongly, rc %lld", what, k, (long long)rc);
        } else {
            Exact<uint16_t> rows(b.rows), out(b.n);
            std::vector<uint16_t> oout(static_cast<size_t>(b.n));
            const int64_t rc = fpcc_simple_dec_pop(d, rows.p, b.n_rows, b.width, out.p, b.n);
            orc_simple_dec_pop(od, b.rows.data(), b.n_rows, b.width, oout.data(), b.n);
            if (rc != OK || out.vec() != b.sym || oout != b.sym) msg = fmt("%s: block %zu (width %lld) decodes wrongly, rc %lld", what, k, (long long)b.width, (long long)rc);
        }
        uint32_t state = 0;
        int64_t pos = -1;
        const OrcDecView *view = reinterpret_cast<const OrcDecView *>(od);
        if (msg.empty() && (fpcc_simple_dec_tell(d, &state, &pos) != OK || pos != view->p - got.data() || state != view->x))
            msg = fmt("%s: after block %zu the decoder stands at %lld (state %u), the oracle at %lld (state %u)", what, k, (long long)pos, state,
                      (long long)(view->p - got.data()), view->x);
    }
    orc_simple_dec_free(od);
    fpcc_simple_dec_free(d);
    return msg;
}

// n rows of `width` strictly increasing edges; every third row has frequency-1 symbols at the first, a middle and the last position
std::vector<uint16_t> rand_rows(Rng &rng, int64_t n, int64_t width) {
    std::vector<uint16_t> rows(static_cast<size_t>(n * width));
    for (int64_t i = 0; i < n; ++i) {
        uint16_t *row = rows.data() + i * width;
        std::vector<uint32_t> c = rand_cdf(rng, static_cast<int>(width) + 1);           // width + 2 edges: 0, width cuts, 65536
        for (int64_t j = 0; j < width; ++j) row[j] = static_cast<uint16_t>(c[static_cast<size_t>(j) + 1]);
        if (i % 3 == 0 && width >= 2) {
            // edges 1, 2, .. m, then 65535 - k .. 65535: every symbol but symbol m has frequency 1, the last one is [65535, 65536)
            const int64_t m = width / 2;
            for (int64_t j = 0; j < width - 1; ++j) row[j] = static_cast<uint16_t>(j < m ? 1 + j : 65535 - (width - 2 - j));
            row[width - 1] = 65535;
        }
    }
    return rows;
}

Block rows_block(Rng &rng, int64_t n, int64_t width, bool one_row, Block::Kind kind) {
    Block b;
    b.kind = kind;
    b.n = n;
    b.width = width;
    b.n_rows = one_row ? 1 : n;
    b.rows = rand_rows(rng, b.n_rows, width);
    b.sym.resize(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) {
        const uint16_t *row = b.rows.data() + (one_row ? 0 : i * width);
        uint32_t s = static_cast<uint32_t>(rng() % static_cast<uint64_t>(width));
        if (i % 4 == 0) s = 0;
        if (i % 4 == 1) s = static_cast<uint32_t>(width / 2 >= 2 ? width / 2 - 1 : width / 2);
        if (i % 4 == 2) s = static_cast<uint32_t>(width - 1);
        uint32_t lo, hi;
        row_range(row, width, s, lo, hi);
        if (hi <= lo) {                                     // (only where rand_rows could not make room) the widest symbol instead
            for (uint32_t c = 0; c < width; ++c) { uint32_t l, h; row_range(row, width, c, l, h); if (h > l) { s = c; break; } }
        }
        b.sym[i] = static_cast<uint16_t>(s);
    }
    return b;
}

Block bin_block(Rng &rng, int64_t n, bool one_row) {
    Block b;
    b.kind = Block::BIN;
    b.n = n;
    b.n_rows = one_row ? 1 : n;
    b.rows.resize(static_cast<size_t>(b.n_rows));
    for (auto &e : b.rows) e = static_cast<uint16_t>(1 + rng() % 65535);
    if (!one_row && n >= 3) { b.rows[0] = 1; b.rows[1] = 65535; }
    b.bits.resize(static_cast<size_t>(n));
    for (auto &v : b.bits) v = static_cast<uint8_t>(rng() & 1);
    if (!one_row && n >= 3) { b.bits[0] = 0; b.bits[1] = 1; }            // the two frequency-1 symbols
    return b;
}

// =================================================================================================================================
// golden replay
// =================================================================================================================================
struct Tokens {
    std::vector<std::string> t;
    size_t at = 0;
    bool done() const { return at >= t.size(); }
    const std::string &next() { static const std::string none; return at < t.size() ? t[at++] : none; }
    int64_t i64() { return std::strtoll(next().c_str(), nullptr, 10); }
    double f64() { return std::strtod(next().c_str(), nullptr); }
    Bytes hex() {
        const std::string &s = next();
        Bytes b(s.size() / 2);
        for (size_t i = 0; i < b.size(); ++i) b[i] = static_cast<uint8_t>(std::strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16));
        return b;
    }
    template <class T> std::vector<T> ints(int64_t n) {
        std::vector<T> v(static_cast<size_t>(n));
        for (auto &x : v) x = static_cast<T>(i64());
        return v;
    }
};

std::string g_golden_path;
std::map<std::string, int> g_replayed;

std::string replay_cdf(Tokens &tk) {
    const int overflow = static_cast<int>(tk.i64());
    const int32_t offset_in = static_cast<int32_t>(tk.i64());
    const int64_t B = tk.i64(), S = tk.i64();
    std::vector<std::vector<double>> pmf(static_cast<size_t>(B));
    for (auto &row : pmf) { row.resize(static_cast<size_t>(S)); for (auto &v : row) v = tk.f64(); }
    const std::vector<int32_t> offset_out = tk.ints<int32_t>(B);
    for (int64_t b = 0; b < B; ++b) {
        const std::vector<uint32_t> want = tk.ints<uint32_t>(tk.i64());
        Exact<double> p(pmf[b]);
        Exact<uint32_t> cdf(S + 2);
        Exact<int32_t> off(1);
        off.p[0] = offset_in;
        const int64_t len = fpcc_pmf_to_quantized_cdf(p.p, S, overflow, off.p, cdf.p);
        REQUIRE(len == static_cast<int64_t>(want.size()), "row %lld: length %lld, golden %zu", (long long)b, (long long)len, want.size());
        REQUIRE(std::equal(want.begin(), want.end(), cdf.p), "row %lld: cdf differs from the golden one", (long long)b);
        REQUIRE(off.p[0] == offset_out[b], "row %lld: offset %d, golden %d", (long long)b, off.p[0], offset_out[b]);
        std::vector<double> clobbered = pmf[b];
        std::vector<uint32_t> ocdf(static_cast<size_t>(S) + 2);
        int32_t ooff = offset_in;
        const int64_t olen = orc_pmf_to_cdf(clobbered.data(), S, overflow, &ooff, ocdf.data());
        REQUIRE(olen == len && std::equal(want.begin(), want.end(), ocdf.begin()) && ooff == off.p[0], "row %lld: oracle differs", (long long)b);
    }
    return "";
}

std::string replay_indexed(Tokens &tk) {
    const int overflow = static_cast<int>(tk.i64());
    const bool with_index = tk.i64() != 0;
    const int64_t n_tables = tk.i64(), n = tk.i64();
    std::vector<std::vector<uint32_t>> rows(static_cast<size_t>(n_tables));
    for (auto &r : rows) r = tk.ints<uint32_t>(tk.i64());
    const std::vector<int32_t> off = tk.ints<int32_t>(n_tables);
    const std::vector<int32_t> sym = tk.ints<int32_t>(n), index = tk.ints<int32_t>(n);
    const Bytes want = tk.hex();
    const Tab t = make_tab(rows, off);
    Bytes got;
    const int64_t cap = overflow ? 40 * n + 64 : 4 * n + 64;
    const int64_t len = lib_idx_enc(t, sym, with_index ? &index : nullptr, overflow, cap, got);
    REQUIRE(len == static_cast<int64_t>(want.size()) && got == want, "stream of %lld bytes, golden %zu", (long long)len, want.size());
    std::vector<int32_t> back;
    EXPECT_RC(lib_idx_dec(t, want, with_index ? &index : nullptr, n, overflow, back), OK, "decode");
    REQUIRE(back == sym, "decode differs");
    return "";
}

std::string replay_binary(Tokens &tk) {
    const int64_t n = tk.i64();
    const std::vector<uint16_t> prob = tk.ints<uint16_t>(n);
    const std::vector<uint8_t> bits = tk.ints<uint8_t>(n);
    const Bytes want = tk.hex();
    for (int64_t cap : {4 * n + 64, 2 * n + 8, 2 * n + 7}) {
        Bytes got;
        const int64_t len = lib_bin_enc(bits, prob, cap, got);
        REQUIRE(len == static_cast<int64_t>(want.size()) && got == want, "cap %lld: stream of %lld bytes, golden %zu", (long long)cap, (long long)len, want.size());
    }
    std::vector<uint8_t> back;
    EXPECT_RC(lib_bin_dec(want, prob, back), OK, "decode");
    REQUIRE(back == bits, "decode differs");
    return "";
}

std::string replay_simple(Tokens &tk, bool bin) {
    std::vector<Block> blocks;
    if (bin) {
        Block b;
        b.kind = Block::BIN;
        b.n_rows = tk.i64();
        b.n = tk.i64();
        b.rows = tk.ints<uint16_t>(b.n_rows);
        b.bits = tk.ints<uint8_t>(b.n);
        blocks.push_back(b);
    } else {
        const int64_t n_blocks = tk.i64();
        for (int64_t k = 0; k < n_blocks; ++k) {
            Block b;
            b.n_rows = tk.i64();
            b.width = tk.i64();
            b.n = tk.i64();
            b.rows = tk.ints<uint16_t>(b.n_rows * b.width);
            b.sym = tk.ints<uint16_t>(b.n);
            blocks.push_back(b);
        }
    }
    const Bytes want = tk.hex();
    REQUIRE(orc_simple_stream(blocks, 1 << 20) == want, "the oracle's stream differs from the golden one");
    PROPAGATE(simple_differential(blocks, "golden"));          // library == oracle == golden, popped in reverse
    if (!bin) {                                                // the same stream through the resolved-range entry point
        for (auto &b : blocks) b.kind = Block::RANGES;
        PROPAGATE(simple_differential(blocks, "golden, as ranges"));
    }
    return "";
}

std::string replay_random(Tokens &tk) {
    const int64_t n = tk.i64();
    const std::vector<uint16_t> prob = tk.ints<uint16_t>(n);
    const std::string bit_string = tk.next();
    REQUIRE(static_cast<int64_t>(bit_string.size()) == n, "bit string of %zu", bit_string.size());
    std::vector<uint8_t> bits(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) bits[i] = bit_string[i] == '1';
    const Bytes want_bin = tk.hex();
    const int64_t n_hist = tk.i64();
    std::vector<double> hist(static_cast<size_t>(n_hist));
    for (auto &v : hist) v = tk.f64();
    const int32_t offset = static_cast<int32_t>(tk.i64());
    const std::vector<int32_t> sym = tk.ints<int32_t>(n);
    const std::vector<uint32_t> want_cdf = tk.ints<uint32_t>(tk.i64());
    const Bytes want_idx = tk.hex();
    Bytes got;
    REQUIRE(lib_bin_enc(bits, prob, 4 * n + 64, got) == static_cast<int64_t>(want_bin.size()) && got == want_bin, "binary stream differs");
    std::vector<uint8_t> back_bits;
    REQUIRE(lib_bin_dec(want_bin, prob, back_bits) == OK && back_bits == bits, "binary decode differs");
    Exact<double> p(hist);
    Exact<uint32_t> cdf(n_hist + 2);
    const int64_t len = fpcc_pmf_to_quantized_cdf(p.p, n_hist, 0, nullptr, cdf.p);
    REQUIRE(len == static_cast<int64_t>(want_cdf.size()) && std::equal(want_cdf.begin(), want_cdf.end(), cdf.p), "cdf differs");
    const Tab t = make_tab({want_cdf}, {offset});
    REQUIRE(lib_idx_enc(t, sym, nullptr, 0, 4 * n + 64, got) == static_cast<int64_t>(want_idx.size()) && got == want_idx, "indexed stream differs");
    std::vector<int32_t> back;
    REQUIRE(lib_idx_dec(t, want_idx, nullptr, n, 0, back) == OK && back == sym, "indexed decode differs");
    return "";
}

std::string check_golden_replay() {
    std::ifstream in(g_golden_path);
    REQUIRE(in.good(), "cannot read %s", g_golden_path.c_str());
    Tokens tk;
    for (std::string s; in >> s;) tk.t.push_back(s);
    while (!tk.done()) {
        const std::string kind = tk.next();
        std::string msg;
        if (kind == "cdf") msg = replay_cdf(tk);
        else if (kind == "indexed") msg = replay_indexed(tk);
        else if (kind == "binary") msg = replay_binary(tk);
        else if (kind == "simple") msg = replay_simple(tk, false);
        else if (kind == "simplebin") msg = replay_simple(tk, true);
        else if (kind == "random") msg = replay_random(tk);
        else return "unknown record '" + kind + "'";
        const int k = ++g_replayed[kind];
        if (!msg.empty()) return fmt("%s case %d: ", kind.c_str(), k - 1) + msg;
        REQUIRE(tk.next() == "end", "%s case %d: record not consumed to its end", kind.c_str(), k - 1);
    }
    return "";
}

// =================================================================================================================================
// differential against the oracle
// =================================================================================================================================
std::string check_binary_differential() {
    Rng rng(101);
    for (int64_t n : {0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 70000}) {
        std::vector<uint8_t> bits;
        std::vector<uint16_t> prob;
        rand_binary(rng, n, bits, prob);
        const Bytes want = orc_bin_enc(bits, prob);
        REQUIRE(want.size() >= 4, "n %lld: the oracle wrote nothing", (long long)n);
        for (int64_t cap : {2 * n + 8, 2 * n + 7}) {          // the branch-free step, the loop
            Bytes got;
            const int64_t len = lib_bin_enc(bits, prob, cap, got);
            REQUIRE(len == static_cast<int64_t>(want.size()) && got == want, "n %lld cap %lld: %lld bytes, the oracle %zu", (long long)n, (long long)cap,
                    (long long)len, want.size());
        }
        std::vector<uint8_t> back, oback(static_cast<size_t>(n));
        EXPECT_RC(lib_bin_dec(want, prob, back), OK, "n %lld", (long long)n);
        REQUIRE(back == bits, "n %lld: decode differs", (long long)n);
        std::vector<uint32_t> p32(prob.begin(), prob.end());
        orc_binary_decode(want.data(), p32.data(), n, oback.data());
        REQUIRE(oback == bits, "n %lld: oracle decode differs", (long long)n);
    }
    return "";
}

std::string check_binary_multi() {
    Rng rng(102);
    const std::vector<int64_t> sizes{0, 5, 1000, 64, 3000};
    std::vector<int64_t> start{0};
    for (int64_t s : sizes) start.push_back(start.back() + s);
    std::vector<uint8_t> bits;
    std::vector<uint16_t> prob;
    rand_binary(rng, start.back(), bits, prob);
    for (int threads : {1, 3}) {
        const int64_t cap = 2 * 3000 + 8, ns = static_cast<int64_t>(sizes.size());
        Exact<uint8_t> b(bits), out(cap * ns);
        Exact<uint16_t> p(prob);
        Exact<int64_t> st(start), len(ns);
        EXPECT_RC(fpcc_rans_binary_encode_multi(b.p, p.p, st.p, ns, out.p, cap, len.p, threads), OK, "%d threads", threads);
        for (int64_t s = 0; s < ns; ++s) {
            const Bytes want = orc_bin_enc(std::vector<uint8_t>(bits.begin() + start[s], bits.begin() + start[s + 1]),
                                           std::vector<uint16_t>(prob.begin() + start[s], prob.begin() + start[s + 1]));
            REQUIRE(len.p[s] == static_cast<int64_t>(want.size()) && std::equal(want.begin(), want.end(), out.p + (s + 1) * cap - len.p[s]),
                    "stream %lld differs from the oracle's", (long long)s);
        }
    }
    return "";
}

std::string check_indexed_differential() {
    Rng rng(103);
    for (int overflow : {0, 1})
        for (int n_tables : {1, 7})
            for (int with_index : {0, 1}) {
                std::vector<std::vector<uint32_t>> rows;
                std::vector<int32_t> off;
                for (int t = 0; t < n_tables; ++t) {
                    rows.push_back(rand_cdf(rng, 2 + static_cast<int>(rng() % 40)));
                    off.push_back(static_cast<int32_t>(rng() % 21) - 10);
                }
                const Tab t = make_tab(rows, off);
                const int64_t n = 1500;
                std::vector<int32_t> sym(n), index(n);
                for (int64_t i = 0; i < n; ++i) {
                    index[i] = static_cast<int32_t>(rng() % static_cast<uint64_t>(n_tables));
                    const int64_t ti = with_index ? index[i] : i % n_tables;
                    const int bins = static_cast<int>(t.len[ti]) - 1;
                    sym[i] = off[ti] + static_cast<int32_t>(rng() % static_cast<uint64_t>(bins));
                    if (overflow && rng() % 5 == 0) sym[i] = off[ti] + static_cast<int32_t>(rng() % 4001) - 2000;
                }
                PROPAGATE(idx_differential(t, sym, with_index ? &index : nullptr, overflow,
                                           fmt("overflow %d, %d tables, index %d", overflow, n_tables, with_index).c_str()));
            }
    return "";
}

// one table, no overflow: the slot lookup table takes over at 8192 symbols, and holds bins as uint16
std::string check_indexed_single_table() {
    Rng rng(104);
    const Tab small = make_tab({rand_cdf(rng, 33)}, {-5});
    for (int64_t n : {8191, 8192, 8193}) {
        std::vector<int32_t> sym(static_cast<size_t>(n));
        for (auto &s : sym) s = -5 + static_cast<int32_t>(rng() % 33);
        PROPAGATE(idx_differential(small, sym, nullptr, 0, fmt("33 bins, n %lld", (long long)n).c_str()));
    }
    // 65535 bins (the last of width 2) and 65536 bins (every slot its own bin: too many for the lookup table's uint16)
    for (int bins : {65535, 65536}) {
        std::vector<uint32_t> c(static_cast<size_t>(bins) + 1);
        for (int i = 0; i < bins; ++i) c[i] = static_cast<uint32_t>(i);
        c[bins] = 65536;
        const Tab wide = make_tab({c}, {7});
        for (int64_t n : {200, 8200}) {
            std::vector<int32_t> sym(static_cast<size_t>(n));
            for (auto &s : sym) s = 7 + static_cast<int32_t>(rng() % static_cast<uint64_t>(bins));
            sym[0] = 7;
            sym[1] = 7 + bins - 1;
            sym[2] = 7 + bins - 2;
            PROPAGATE(idx_differential(wide, sym, nullptr, 0, fmt("%d bins, n %lld", bins, (long long)n).c_str()));
        }
    }
    // two bins, with and without the escape (where the second bin is the escape bin), and the one-bin tables
    for (uint32_t cut : {1u, 32768u, 65535u})
        for (int overflow : {0, 1}) {
            const Tab two = make_tab({{0, cut, 65536}}, {3});
            std::vector<int32_t> sym(600);
            for (auto &s : sym) s = 3 + static_cast<int32_t>(rng() % 2) + (overflow ? static_cast<int32_t>(rng() % 9) - 4 : 0);
            PROPAGATE(idx_differential(two, sym, nullptr, overflow, fmt("two bins cut at %u, overflow %d", cut, overflow).c_str()));
        }
    for (int overflow : {0, 1}) {
        const Tab one = make_tab({{0, 65536}}, {-2});
        std::vector<int32_t> sym(50, -2);
        if (overflow) for (auto &s : sym) s = static_cast<int32_t>(rng() % 2001) - 1000;          // the escape bin alone
        PROPAGATE(idx_differential(one, sym, nullptr, overflow, fmt("one bin, overflow %d", overflow).c_str()));
    }
    return "";
}

// escape values up to the ends of int32.  The oracle keeps magnitudes in int32 (its encoder negates the difference, its decoder
// forms magnitude + escape bin before it subtracts 1), so it is defined for differences in [INT32_MIN + 1, INT32_MAX - 1]; the
// differences INT32_MIN and INT32_MAX are checked as round trips of the library alone, a difference outside int32 must be refused.
std::string g_escape_note;
std::string check_escape_values() {
    const std::vector<uint32_t> cdf{0, 100, 30000, 50000, 65000, 65536};        // 4 bins + the escape bin: esc = 4
    const int64_t esc = 4;
    std::vector<int64_t> values{0, 1, -1, esc - 1, esc, esc + 1, INT32_MAX, int64_t(INT32_MIN) + 1, INT32_MIN};
    for (int k = 1; k <= 30; ++k)
        for (int64_t d : {-1, 0, 1}) { values.push_back((int64_t(1) << k) + d); values.push_back(-((int64_t(1) << k) + d)); }
    std::string lib_only, refused;
    for (int32_t offset : {0, 1000, -1000}) {
        const Tab t = make_tab({cdf}, {offset});
        std::vector<int32_t> with_oracle, lib_alone;
        std::vector<int64_t> symbols = values;                         // each value as the symbol and as the coded difference
        for (int64_t v : values) if (offset != 0 && v + offset >= INT32_MIN && v + offset <= INT32_MAX) symbols.push_back(v + offset);
        for (int64_t sym : symbols) {
            const int64_t diff = sym - offset;
            if (diff < INT32_MIN || diff > INT32_MAX) {
                Bytes got;
                EXPECT_RC(lib_idx_enc(t, {0, static_cast<int32_t>(sym), 1}, nullptr, 1, 256, got), E_ARG, "symbol %lld, offset %d", (long long)sym, offset);
                refused += fmt(" %lld-(%d)", (long long)sym, offset);
                continue;
            }
            if (diff == INT32_MIN || diff == INT32_MAX) { lib_alone.push_back(static_cast<int32_t>(sym)); lib_only += fmt(" %lld-(%d)", (long long)sym, offset); continue; }
            with_oracle.push_back(static_cast<int32_t>(sym));
            PROPAGATE(idx_differential(t, {static_cast<int32_t>(sym)}, nullptr, 1, fmt("symbol %lld, offset %d", (long long)sym, offset).c_str()));
        }
        PROPAGATE(idx_differential(t, with_oracle, nullptr, 1, fmt("all values in one stream, offset %d", offset).c_str()));
        // also the values whose difference fits in int32 relative to the other two symbols of this table: the same tables, indexed
        for (int32_t sym : lib_alone) {
            std::vector<int32_t> three{offset + 2, sym, offset - 7}, back;
            Bytes got;
            REQUIRE(lib_idx_enc(t, three, nullptr, 1, 40 * 3 + 64, got) >= 4, "symbol %d, offset %d: encode refused", sym, offset);
            EXPECT_RC(lib_idx_dec(t, got, nullptr, 3, 1, back), OK, "symbol %d, offset %d", sym, offset);
            REQUIRE(back == three, "symbol %d, offset %d: round trip gives %d", sym, offset, back[1]);
        }
        // every value the library takes, in one stream, round trip of the library alone
        std::vector<int32_t> all = with_oracle, back;
        all.insert(all.end(), lib_alone.begin(), lib_alone.end());
        Bytes got;
        REQUIRE(lib_idx_enc(t, all, nullptr, 1, 40 * static_cast<int64_t>(all.size()) + 64, got) >= 4, "offset %d: encode of all values refused", offset);
        REQUIRE(lib_idx_dec(t, got, nullptr, static_cast<int64_t>(all.size()), 1, back) == OK && back == all, "offset %d: round trip of all values differs", offset);
    }
    g_escape_note = "symbol-(offset) checked by the library alone:" + lib_only + "; refused (difference outside int32):" + refused;
    return "";
}

std::string check_simple_differential() {
    Rng rng(105);
    for (int64_t width : {1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 300}) {
        const int64_t n = 48;
        std::vector<Block> blocks;
        blocks.push_back(rows_block(rng, n, width, false, Block::ROWS));
        blocks.push_back(bin_block(rng, 37, false));
        blocks.push_back(rows_block(rng, n, width, true, Block::ROWS));
        blocks.push_back(rows_block(rng, n, width, false, Block::RANGES));
        blocks.push_back(bin_block(rng, 21, true));
        blocks.push_back(rows_block(rng, 5, width, true, Block::RANGES));
        PROPAGATE(simple_differential(blocks, fmt("width %lld", (long long)width).c_str()));
        PROPAGATE(simple_differential({blocks[0]}, fmt("width %lld, one block, n_rows == n", (long long)width).c_str()));
        PROPAGATE(simple_differential({blocks[2]}, fmt("width %lld, one block, n_rows == 1", (long long)width).c_str()));
    }
    // a long block through both steps of push_ranges: the room for the branch-free one (2 bytes per symbol) and not
    const Block big = rows_block(rng, 1500, 255, false, Block::RANGES);
    const Bytes want = orc_simple_stream({big}, 1 << 20);
    for (int64_t buf : {int64_t(2 * 1500 + 8), int64_t(2 * 1500 + 7), static_cast<int64_t>(want.size())}) {
        fpcc_simple_enc *e = fpcc_simple_enc_new(buf);
        REQUIRE(e != nullptr, "no encoder of %lld bytes", (long long)buf);
        const int64_t rc = lib_push(e, big);
        Bytes got;
        const int64_t len = lib_finish(e, static_cast<int64_t>(want.size()), got);
        fpcc_simple_enc_free(e);
        REQUIRE(rc >= 0 && len == static_cast<int64_t>(want.size()) && got == want, "push_ranges into %lld bytes: rc %lld, %lld bytes, the oracle %zu", (long long)buf,
                (long long)rc, (long long)len, want.size());
    }
    return "";
}

std::string check_pmf_differential() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN(), den = 4.9406564584124654e-324;
    std::vector<std::vector<double>> cases{
        {0, 0, 1, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 1},                                 // one-hot
        std::vector<double>(37, 1.0 / 37), std::vector<double>(4, 0.25), std::vector<double>(300, 1.0),      // all equal
        {den, 3 * den, den, 0, 7 * den, den}, {den, 0.5, den, den, 0.25, den, den},       // denormal-heavy
        {1.0}, {0.3}, {2.5}, {den},                                                      // length 1
        {0.5, 0.4, 0.3, 0.2}, {3, 1, 4, 1, 5, 9, 2, 6},                                  // mass above 1
        {0.1, 0.05, 0.2}, {1e-9, 2e-9, 1e-12}, {0.2, 0, 0, 0.1, 0},                      // mass below 1
        {0, 0, 0, 0},                                                                    // all zero: in overflow mode the escape bin takes all
    };
    Rng rng(106);
    for (int k = 0; k < 20; ++k) {
        std::vector<double> p(1 + rng() % 80);
        for (auto &v : p) v = rng() % 4 == 0 ? 0.0 : std::ldexp(static_cast<double>(rng() % 1000), -static_cast<int>(rng() % 30));
        if (std::all_of(p.begin(), p.end(), [](double v) { return v == 0.0; })) p[0] = 1.0;
        cases.push_back(p);
    }
    for (size_t k = 0; k < cases.size(); ++k)
        for (int overflow : {0, 1}) {
            const std::vector<double> &pmf = cases[k];
            const int64_t n = static_cast<int64_t>(pmf.size());
            const bool all_zero = std::all_of(pmf.begin(), pmf.end(), [](double v) { return v == 0.0; });
            Exact<double> p(pmf);
            Exact<uint32_t> cdf(n + 2);
            Exact<int32_t> off(1);
            off.p[0] = -3;
            const int64_t len = fpcc_pmf_to_quantized_cdf(p.p, n, overflow, overflow ? off.p : nullptr, cdf.p);
            if (all_zero && !overflow) { REQUIRE(len == E_ARG, "case %zu: an all-zero pmf returned %lld", k, (long long)len); continue; }
            std::vector<double> clobbered = pmf;
            std::vector<uint32_t> ocdf(static_cast<size_t>(n) + 2);
            int32_t ooff = -3;
            const int64_t olen = orc_pmf_to_cdf(clobbered.data(), n, overflow, &ooff, ocdf.data());
            if (olen < 0) { REQUIRE(len == E_CDF, "case %zu overflow %d: the oracle finds no donor bin, the library returned %lld", k, overflow, (long long)len); continue; }
            REQUIRE(len == olen && std::equal(ocdf.begin(), ocdf.begin() + olen, cdf.p) && (!overflow || off.p[0] == ooff),
                    "case %zu overflow %d: length %lld, the oracle %lld", k, overflow, (long long)len, (long long)olen);
            REQUIRE(std::memcmp(p.p, pmf.data(), pmf.size() * sizeof(double)) == 0, "case %zu: the pmf was written to", k);
        }
    for (int overflow : {0, 1})
        for (double poison : {-0.25, nan, inf, -inf})
            for (size_t at : {size_t(0), size_t(2), size_t(4)}) {
                std::vector<double> pmf{0.1, 0.2, 0.3, 0.2, 0.1};
                pmf[at] = poison;
                Exact<double> p(pmf);
                Exact<uint32_t> cdf(7);
                int32_t off = 0;
                EXPECT_RC(fpcc_pmf_to_quantized_cdf(p.p, 5, overflow, &off, cdf.p), E_ARG, "%g at %zu, overflow %d", poison, at, overflow);
            }
    // more bins than the 16-bit interval has counts: no CDF
    {
        std::vector<double> pmf(70000, 1.0);
        Exact<double> p(pmf);
        Exact<uint32_t> cdf(70002);
        EXPECT_RC(fpcc_pmf_to_quantized_cdf(p.p, 70000, 0, nullptr, cdf.p), E_CDF, "70000 equal bins");
    }
    return "";
}

// =================================================================================================================================
// exact-fit buffers
// =================================================================================================================================
std::string check_exact_fit() {
    Rng rng(107);
    {
        std::vector<uint8_t> bits;
        std::vector<uint16_t> prob;
        const int64_t n = 700;
        rand_binary(rng, n, bits, prob);
        Bytes want, got;
        const int64_t L = lib_bin_enc(bits, prob, 4 * n + 64, want);
        REQUIRE(L > 8 && want == orc_bin_enc(bits, prob), "binary: roomy call returned %lld", (long long)L);
        for (int64_t cap : {L, 2 * n + 8, 2 * n + 7}) { got.clear(); REQUIRE(lib_bin_enc(bits, prob, cap, got) == L && got == want, "binary: cap %lld differs", (long long)cap); }
        for (int64_t cap : {L - 1, int64_t(4), int64_t(3), int64_t(0)}) EXPECT_RC(lib_bin_enc(bits, prob, cap, got), E_BUFFER, "binary, cap %lld", (long long)cap);
        // an empty stream is its state: exactly 4 bytes
        REQUIRE(lib_bin_enc({}, {}, 4, got) == 4 && got == Bytes({0, 0, 0x80, 0}), "binary: the empty stream in 4 bytes");
        EXPECT_RC(lib_bin_enc({}, {}, 3, got), E_BUFFER, "binary: the empty stream in 3 bytes");
        EXPECT_RC(lib_bin_enc({}, {}, 0, got), E_BUFFER, "binary: the empty stream in 0 bytes");
    }
    for (int overflow : {0, 1}) {
        const Tab t = make_tab({rand_cdf(rng, 9), rand_cdf(rng, 30)}, {0, -4});
        std::vector<int32_t> sym(400);
        for (size_t i = 0; i < sym.size(); ++i) {
            const int bins = i % 2 ? 30 : 9;
            sym[i] = (i % 2 ? -4 : 0) + static_cast<int32_t>(rng() % static_cast<uint64_t>(bins)) + (overflow && i % 7 == 0 ? 5000 - static_cast<int32_t>(rng() % 10000) : 0);
        }
        Bytes want, got;
        const int64_t L = lib_idx_enc(t, sym, nullptr, overflow, 40 * 400 + 64, want);
        REQUIRE(L > 8 && want == orc_idx_enc(t, sym, nullptr, overflow), "indexed, overflow %d: roomy call returned %lld", overflow, (long long)L);
        REQUIRE(lib_idx_enc(t, sym, nullptr, overflow, L, got) == L && got == want, "indexed, overflow %d: cap == L differs", overflow);
        for (int64_t cap : {L - 1, int64_t(4), int64_t(3), int64_t(0)}) EXPECT_RC(lib_idx_enc(t, sym, nullptr, overflow, cap, got), E_BUFFER, "indexed, overflow %d, cap %lld", overflow, (long long)cap);
    }
    {
        const std::vector<Block> blocks{rows_block(rng, 300, 255, false, Block::ROWS), bin_block(rng, 100, false), rows_block(rng, 200, 40, true, Block::RANGES)};
        const Bytes want = orc_simple_stream(blocks, 1 << 16);
        const int64_t L = static_cast<int64_t>(want.size());
        // the encoder's own buffer: exactly L bytes hold the stream, L - 1 do not
        for (int64_t buf : {int64_t(1 << 16), L, L - 1}) {
            for (int64_t cap : {L, L - 1, int64_t(4), int64_t(3), int64_t(0)}) {
                fpcc_simple_enc *e = fpcc_simple_enc_new(buf);
                REQUIRE(e != nullptr, "simple: no encoder of %lld bytes", (long long)buf);
                int64_t rc = 0;
                for (const Block &b : blocks) rc = lib_push(e, b);
                Bytes got;
                const int64_t len = lib_finish(e, cap, got);
                if (buf >= L && cap >= L) {
                    if (rc != L - 4 || len != L || got != want) { fpcc_simple_enc_free(e); return fmt("simple: buffer %lld, cap %lld: push %lld, finish %lld", (long long)buf, (long long)cap, (long long)rc, (long long)len); }
                } else if (len != E_BUFFER) {
                    fpcc_simple_enc_free(e);
                    return fmt("simple: buffer %lld, cap %lld: push %lld, finish %lld, expected E_BUFFER", (long long)buf, (long long)cap, (long long)rc, (long long)len);
                }
                // finish has reset the encoder, whatever it returned: the next stream is a new encoder's
                const int64_t rc2 = lib_push(e, blocks[1]);
                const int64_t len2 = lib_finish(e, 1 << 16, got);
                fpcc_simple_enc_free(e);
                REQUIRE(rc2 >= 0 && len2 >= 4 && got == orc_simple_stream({blocks[1]}, 1 << 16), "simple: buffer %lld, cap %lld: the stream after finish differs", (long long)buf, (long long)cap);
            }
        }
    }
    return "";
}

// =================================================================================================================================
// error paths
// =================================================================================================================================
std::string check_err_binary_zero_probability() {
    Rng rng(108);
    const int64_t n = 101;
    for (int64_t at : {int64_t(0), n / 2, n - 1})
        for (int bit : {0, 1})
            for (int64_t cap : {2 * n + 8, 2 * n + 7, 4 * n + 64}) {
                std::vector<uint8_t> bits;
                std::vector<uint16_t> prob;
                rand_binary(rng, n, bits, prob);
                prob[at] = 0;
                bits[at] = static_cast<uint8_t>(bit);
                Bytes got;
                EXPECT_RC(lib_bin_enc(bits, prob, cap, got), E_ARG, "zero at %lld, bit %d, cap %lld", (long long)at, bit, (long long)cap);
            }
    // the same through the multi-stream entry: the stream with the zero is refused, the other one is coded
    std::vector<uint8_t> bits;
    std::vector<uint16_t> prob;
    rand_binary(rng, 2 * n, bits, prob);
    prob[n + 7] = 0;
    bits[n + 7] = 0;
    const int64_t cap = 2 * n + 8;
    Exact<uint8_t> b(bits), out(2 * cap);
    Exact<uint16_t> p(prob);
    Exact<int64_t> st(std::vector<int64_t>{0, n, 2 * n}), len(2);
    EXPECT_RC(fpcc_rans_binary_encode_multi(b.p, p.p, st.p, 2, out.p, cap, len.p, 2), E_ARG, "multi");
    const Bytes want = orc_bin_enc(std::vector<uint8_t>(bits.begin(), bits.begin() + n), std::vector<uint16_t>(prob.begin(), prob.begin() + n));
    REQUIRE(len.p[1] == E_ARG && len.p[0] == static_cast<int64_t>(want.size()) && std::equal(want.begin(), want.end(), out.p + cap - len.p[0]),
            "multi: lengths %lld, %lld", (long long)len.p[0], (long long)len.p[1]);
    return "";
}

std::string check_err_multi_start() {
    std::vector<uint8_t> bits(100, 1);
    std::vector<uint16_t> prob(100, 40000);
    Exact<uint8_t> b(bits), out(3 * 300);
    Exact<uint16_t> p(prob);
    Exact<int64_t> len(3);
    for (const std::vector<int64_t> &start : {std::vector<int64_t>{0, 60, 40, 100}, std::vector<int64_t>{0, 50, 100, 90}, std::vector<int64_t>{-1, 50, 60, 100},
                                              std::vector<int64_t>{10, 0, 50, 100}}) {
        Exact<int64_t> st(start);
        for (int threads : {1, 2}) EXPECT_RC(fpcc_rans_binary_encode_multi(b.p, p.p, st.p, 3, out.p, 300, len.p, threads), E_ARG, "start %lld %lld %lld %lld",
                                             (long long)start[0], (long long)start[1], (long long)start[2], (long long)start[3]);
    }
    Exact<int64_t> st(std::vector<int64_t>{0, 0, 100, 100});
    EXPECT_RC(fpcc_rans_binary_encode_multi(b.p, p.p, st.p, 3, out.p, 300, len.p, 2), OK, "empty streams between equal starts");
    REQUIRE(len.p[0] == 4 && len.p[2] == 4 && len.p[1] > 4, "lengths %lld %lld %lld", (long long)len.p[0], (long long)len.p[1], (long long)len.p[2]);
    return "";
}

// after a failed push: finish is safe, and the encoder then writes what a new encoder writes
std::string after_failed_push(fpcc_simple_enc *e, Rng &rng, const char *what) {
    Bytes got;
    (void)lib_finish(e, 1 << 16, got);
    const std::vector<Block> fresh{rows_block(rng, 60, 17, false, Block::ROWS), bin_block(rng, 30, false)};
    for (const Block &b : fresh) EXPECT_RC(lib_push(e, b) < 0 ? -1 : 0, 0, "%s: push after the failed one", what);
    const int64_t len = lib_finish(e, 1 << 16, got);
    REQUIRE(len >= 4 && got == orc_simple_stream(fresh, 1 << 16), "%s: the stream after a failed push differs from a new encoder's (%lld bytes)", what, (long long)len);
    return "";
}

std::string check_err_simple_push() {
    Rng rng(109);
    {
        fpcc_simple_enc *e = fpcc_simple_enc_new(1 << 16);
        REQUIRE(e != nullptr, "no encoder");
        std::string msg;
        auto bail = [&](const std::string &m) { fpcc_simple_enc_free(e); return m; };
        const int64_t n = 40, width = 9;
        for (int64_t at : {int64_t(0), n / 2, n - 1}) {
            // symbol >= width
            Block b = rows_block(rng, n, width, false, Block::ROWS);
            const Block ok = rows_block(rng, 10, width, true, Block::ROWS);
            if (lib_push(e, ok) < 0) return bail("valid push refused");
            b.sym[at] = static_cast<uint16_t>(width);
            if (lib_push(e, b) != E_ARG) return bail(fmt("symbol == width at %lld accepted", (long long)at));
            if (!(msg = after_failed_push(e, rng, "symbol == width")).empty()) return bail(msg);
            b.sym[at] = 65535;
            if (lib_push(e, b) != E_ARG) return bail(fmt("symbol 65535 at %lld accepted", (long long)at));
            if (!(msg = after_failed_push(e, rng, "symbol 65535")).empty()) return bail(msg);
            // a row that does not increase at the coded symbol (the last symbol ends at 65536 whatever the row says: it always has a range)
            for (int64_t sy : {int64_t(0), width / 2, width - 2}) {
                b = rows_block(rng, n, width, false, Block::ROWS);
                uint16_t *row = b.rows.data() + at * width;
                b.sym[at] = static_cast<uint16_t>(sy);
                row[sy] = sy ? row[sy - 1] : 0;                                              // flat
                if (lib_push(e, ok) < 0) return bail("valid push refused");
                if (lib_push(e, b) != E_ARG) return bail(fmt("flat row at symbol %lld of row %lld accepted", (long long)sy, (long long)at));
                if (!(msg = after_failed_push(e, rng, "flat row")).empty()) return bail(msg);
                if (sy > 0) {
                    row[sy] = static_cast<uint16_t>(row[sy - 1] - 1);                        // decreasing
                    if (lib_push(e, b) != E_ARG) return bail(fmt("decreasing row at symbol %lld of row %lld accepted", (long long)sy, (long long)at));
                    if (!(msg = after_failed_push(e, rng, "decreasing row")).empty()) return bail(msg);
                }
            }
            // push_bin: a zero under an edge of 0 has no range; a one under it has all of it
            Block bin = bin_block(rng, n, false);
            bin.rows[at] = 0;
            bin.bits[at] = 1;
            if (lib_push(e, ok) < 0 || lib_push(e, bin) < 0) return bail("push_bin: a one above edge 0 refused");
            Bytes got;
            if (lib_finish(e, 1 << 16, got) < 4 || got != orc_simple_stream({ok, bin}, 1 << 16)) return bail("push_bin: edge 0 and a one differs from the oracle");
            bin.bits[at] = 0;
            if (lib_push(e, ok) < 0) return bail("valid push refused");
            const int64_t rc = lib_push(e, bin);
            if (rc != E_ARG) return bail(fmt("push_bin: edge 0 and a zero at %lld returned %lld, expected E_ARG", (long long)at, (long long)rc));
            if (!(msg = after_failed_push(e, rng, "push_bin edge 0")).empty()) return bail(msg);
            bin = bin_block(rng, n, true);
            bin.rows[0] = 0;
            bin.bits.assign(static_cast<size_t>(n), 1);
            bin.bits[at] = 0;
            if (lib_push(e, bin) != E_ARG) return bail("push_bin: one shared edge 0 and a zero accepted");
            if (!(msg = after_failed_push(e, rng, "push_bin shared edge 0")).empty()) return bail(msg);
        }
        fpcc_simple_enc_free(e);
    }
    // push_bin on a fresh small encoder: the refusal must not have flooded the buffer
    {
        fpcc_simple_enc *e = fpcc_simple_enc_new(4096);
        REQUIRE(e != nullptr, "no encoder");
        Exact<uint16_t> edge(std::vector<uint16_t>{30000, 0, 30000});
        Exact<uint8_t> bits(std::vector<uint8_t>{1, 0, 0});
        const int64_t rc = fpcc_simple_enc_push_bin(e, edge.p, 3, bits.p, 3);
        fpcc_simple_enc_free(e);
        EXPECT_RC(rc, E_ARG, "push_bin with edge == 0 and a zero bit on a fresh 4 KB encoder");
    }
    return "";
}

std::string check_err_push_ranges() {
    Rng rng(110);
    const int64_t n = 20;
    for (int64_t buf : {int64_t(1 << 16), 2 * n + 8, 2 * n + 7}) {             // branch-free step, exactly its room, the loop
        for (int64_t at : {int64_t(0), n / 2, n - 1}) {
            fpcc_simple_enc *e = fpcc_simple_enc_new(buf);
            REQUIRE(e != nullptr, "no encoder");
            std::vector<uint16_t> start(static_cast<size_t>(n)), fm1(static_cast<size_t>(n));
            for (int64_t i = 0; i < n; ++i) { start[i] = static_cast<uint16_t>(rng() % 60000); fm1[i] = static_cast<uint16_t>(rng() % (65536 - start[i])); }
            for (const auto &bad : {std::pair<int, int>{60000, 9999}, std::pair<int, int>{65535, 1}, std::pair<int, int>{1, 65535}, std::pair<int, int>{65535, 65535}}) {
                std::vector<uint16_t> s = start, f = fm1;
                s[at] = static_cast<uint16_t>(bad.first);
                f[at] = static_cast<uint16_t>(bad.second);
                Exact<uint16_t> sp(s), fp(f);
                const int64_t rc = fpcc_simple_enc_push_ranges(e, sp.p, fp.p, n);
                if (rc != E_ARG) { fpcc_simple_enc_free(e); return fmt("buffer %lld: range %d + %d + 1 at %lld returned %lld, expected E_ARG", (long long)buf, bad.first, bad.second, (long long)at, (long long)rc); }
                Bytes drop;
                (void)lib_finish(e, 1 << 16, drop);
            }
            // the widest ranges that do fit: [0, 65536), [65535, 65536), [60000, 65536)
            std::vector<uint16_t> s = start, f = fm1;
            s[at] = 0; f[at] = 65535;
            s[(at + 1) % n] = 65535; f[(at + 1) % n] = 0;
            s[(at + 2) % n] = 60000; f[(at + 2) % n] = 5535;
            Exact<uint16_t> sp(s), fp(f);
            const int64_t rc = fpcc_simple_enc_push_ranges(e, sp.p, fp.p, n);
            Bytes got;
            const int64_t len = lib_finish(e, 1 << 16, got);
            fpcc_simple_enc_free(e);
            REQUIRE(rc >= 0 && len >= 4, "buffer %lld: valid ranges after refused ones: push %lld, finish %lld", (long long)buf, (long long)rc, (long long)len);
            // what a new encoder writes for them: row coding of two-edge rows [start, start + freq) is not expressible, so decode instead
            Exact<uint8_t> stream(got);
            fpcc_simple_dec *d = fpcc_simple_dec_new(stream.p, stream.n);
            REQUIRE(d != nullptr, "buffer %lld: the stream after refused ranges does not open", (long long)buf);
            for (int64_t i = 0; i < n; ++i) {
                // a row [start, start + freq] of width 3 has the coded range as its symbol 1 (symbol 0 where start == 0)
                const uint32_t lo = s[i], hi = lo + f[i] + 1u;
                std::vector<uint16_t> row{static_cast<uint16_t>(lo), static_cast<uint16_t>(hi >= 65536u ? 65535u : hi), 65535};
                uint16_t want = 1;
                if (hi >= 65536u) { row = {static_cast<uint16_t>(lo), 65535}; want = 1; }          // width 2: symbol 1 = [lo, 65536)
                if (lo == 0) { row.erase(row.begin()); want = 0; }
                Exact<uint16_t> r(row), out(1);
                if (fpcc_simple_dec_pop(d, r.p, 1, r.n, out.p, 1) != OK || out.p[0] != want) {
                    fpcc_simple_dec_free(d);
                    return fmt("buffer %lld: symbol %lld of the stream after refused ranges decodes to %u", (long long)buf, (long long)i, out.p[0]);
                }
            }
            uint32_t state = 0;
            int64_t pos = 0;
            fpcc_simple_dec_tell(d, &state, &pos);
            fpcc_simple_dec_free(d);
            REQUIRE(pos == len && state == (1u << 23), "buffer %lld: the decoder ends at %lld of %lld, state %u", (long long)buf, (long long)pos, (long long)len, state);
        }
    }
    return "";
}

// part 0: indices and symbols; part 1: tables too short for any mode; part 2: tables that are no quantised CDF, and one-bin tables
std::string err_indexed(int part) {
    Rng rng(111);
    const std::vector<std::vector<uint32_t>> good{rand_cdf(rng, 6), rand_cdf(rng, 12), rand_cdf(rng, 4)};
    const std::vector<int32_t> off{0, -3, 5};
    const int64_t n = 90;
    auto symbols = [&](const Tab &t, int overflow) {
        std::vector<int32_t> sym(static_cast<size_t>(n));
        for (int64_t i = 0; i < n; ++i) {
            const int bins = std::max<int>(1, static_cast<int>(t.len[i % 3]) - 1 - overflow);
            sym[i] = t.off[i % 3] + static_cast<int32_t>(rng() % static_cast<uint64_t>(bins));
        }
        return sym;
    };
    Bytes got, valid;
    std::vector<int32_t> back;
    for (int overflow : part == 1 ? std::vector<int>{1, 0} : std::vector<int>{0, 1}) {          // (short tables: the escape coder first)
        const Tab t = make_tab(good, off);
        const std::vector<int32_t> sym = symbols(t, overflow);
        REQUIRE(lib_idx_enc(t, sym, nullptr, overflow, 40 * n + 64, valid) >= 4, "valid input refused");
        for (int64_t at : {int64_t(0), n / 2, n - 1}) {
            if (part != 0) break;
            // a table index out of range
            for (int32_t bad : {-1, 3, INT32_MAX, INT32_MIN}) {
                std::vector<int32_t> index(static_cast<size_t>(n));
                for (int64_t i = 0; i < n; ++i) index[i] = static_cast<int32_t>(i % 3);
                index[at] = bad;
                EXPECT_RC(lib_idx_enc(t, sym, &index, overflow, 40 * n + 64, got), E_ARG, "encode, index %d at %lld, overflow %d", bad, (long long)at, overflow);
                EXPECT_RC(lib_idx_dec(t, valid, &index, n, overflow, back), E_ARG, "decode, index %d at %lld, overflow %d", bad, (long long)at, overflow);
            }
            // a symbol its table cannot code
            std::vector<int32_t> s = sym;
            const int bins = static_cast<int>(t.len[at % 3]) - 1;
            for (int64_t v : {int64_t(-1), int64_t(bins)}) {
                s[at] = static_cast<int32_t>(v + t.off[at % 3]);
                const int64_t rc = lib_idx_enc(t, s, nullptr, overflow, 40 * n + 64, got);
                if (!overflow) REQUIRE(rc == E_ARG, "symbol %lld outside a table without overflow at %lld returned %lld", (long long)v, (long long)at, (long long)rc);
                else REQUIRE(rc >= 4 && lib_idx_dec(t, got, nullptr, n, 1, back) == OK && back == s, "escape of %lld at %lld: rc %lld", (long long)v, (long long)at, (long long)rc);
            }
            // symbol - offset that is no int32
            for (const auto &so : {std::pair<int32_t, int32_t>{INT32_MAX, -1}, std::pair<int32_t, int32_t>{INT32_MIN, 1}, std::pair<int32_t, int32_t>{INT32_MIN, INT32_MAX},
                                   std::pair<int32_t, int32_t>{INT32_MAX, INT32_MIN}, std::pair<int32_t, int32_t>{0, INT32_MIN}}) {
                Tab far = t;
                far.off[at % 3] = so.second;
                std::vector<int32_t> s2 = sym;
                for (int64_t i = 0; i < n; ++i) if (i % 3 == at % 3) s2[i] = so.second;        // (offset + 0: the first bin)
                s2[at] = so.first;
                EXPECT_RC(lib_idx_enc(far, s2, nullptr, overflow, 40 * n + 64, got), E_ARG, "symbol %d - offset %d at %lld, overflow %d", so.first, so.second, (long long)at, overflow);
            }
        }
        // malformed tables, as the first, middle and last of three
        for (int which = 0; which < 3 && part != 0; ++which) {
            struct Bad { std::vector<uint32_t> cdf; int64_t want; const char *what; };
            const std::vector<Bad> bads{
                {{1, 500, 65536}, E_CDF, "cdf[0] != 0"}, {{0, 500, 65535}, E_CDF, "last != 65536"}, {{0, 500, 65537}, E_CDF, "last != 65536"},
                {{0, 500, 500, 65536}, E_CDF, "flat"}, {{0, 600, 500, 65536}, E_CDF, "decreasing"}, {{0, 65536, 65536}, E_CDF, "flat at the end"},
                {{0, 0, 65536}, E_CDF, "flat at the start"}, {{0}, E_ARG, "cdf_len 1"}, {{}, E_ARG, "cdf_len 0"}, {{65536}, E_ARG, "cdf_len 1"},
                {{0, 65535}, E_CDF, "cdf_len 2, last != 65536"}, {{5, 65536}, E_CDF, "cdf_len 2, cdf[0] != 0"}, {{65536, 0}, E_CDF, "cdf_len 2, reversed"},
            };
            for (const Bad &bad : bads) {
                if ((bad.cdf.size() < 2) != (part == 1)) continue;
                std::vector<std::vector<uint32_t>> rows = good;
                rows[which] = bad.cdf;
                const Tab t2 = make_tab(rows, off);
                std::vector<int32_t> s = sym;
                for (int64_t i = 0; i < n; ++i) if (i % 3 == which) s[i] = off[which];
                EXPECT_RC(lib_idx_enc(t2, s, nullptr, overflow, 40 * n + 64, got), bad.want, "encode, table %d %s, overflow %d", which, bad.what, overflow);
                EXPECT_RC(lib_idx_dec(t2, valid, nullptr, n, overflow, back), bad.want, "decode, table %d %s, overflow %d", which, bad.what, overflow);
                // the table is checked even where no symbol uses it
                std::vector<int32_t> index(static_cast<size_t>(n), (which + 1) % 3), s3(static_cast<size_t>(n), off[(which + 1) % 3]);
                EXPECT_RC(lib_idx_enc(t2, s3, &index, overflow, 40 * n + 64, got), bad.want, "encode, unused table %d %s, overflow %d", which, bad.what, overflow);
                EXPECT_RC(lib_idx_dec(t2, valid, &index, 0, overflow, back), bad.want, "decode of no symbols, table %d %s, overflow %d", which, bad.what, overflow);
            }
            if (part == 1) continue;
            // cdf_len 2, well formed: one bin -- without overflow the only symbol, with overflow the escape bin alone
            std::vector<std::vector<uint32_t>> rows = good;
            rows[which] = {0, 65536};
            const Tab t2 = make_tab(rows, off);
            std::vector<int32_t> s = sym;
            for (int64_t i = 0; i < n; ++i) if (i % 3 == which) s[i] = off[which] + (overflow ? static_cast<int32_t>(rng() % 41) - 20 : 0);
            PROPAGATE(idx_differential(t2, s, nullptr, overflow, fmt("table %d with cdf_len 2, overflow %d", which, overflow).c_str()));
            if (!overflow) { s[which] = off[which] + 1; EXPECT_RC(lib_idx_enc(t2, s, nullptr, 0, 40 * n + 64, got), E_ARG, "second symbol of a one-bin table"); }
        }
    }
    return "";
}

std::string check_err_indexed_symbols() { return err_indexed(0); }
std::string check_err_indexed_short_tables() { return err_indexed(1); }
std::string check_err_indexed_malformed_tables() { return err_indexed(2); }

std::string check_err_null_and_negative() {
    uint8_t b8[64] = {0};
    uint16_t b16[64];
    int32_t i32[16] = {0};
    int64_t i64v[4] = {0, 3, 3, 3};
    uint32_t cdf[3] = {0, 30000, 65536};
    double pmf[2] = {0.5, 0.5};
    for (auto &v : b16) v = 30000;
    int64_t start0 = 0, len3 = 3, out64 = 0;
    uint32_t flag = 0, state = 0;
#define ARG(expr) EXPECT_RC((expr), E_ARG, "null or negative argument")
    ARG(fpcc_pmf_to_quantized_cdf(nullptr, 2, 0, nullptr, cdf));
    ARG(fpcc_pmf_to_quantized_cdf(pmf, 2, 0, nullptr, nullptr));
    ARG(fpcc_pmf_to_quantized_cdf(pmf, 2, 1, nullptr, cdf));
    ARG(fpcc_pmf_to_quantized_cdf(pmf, 0, 0, nullptr, cdf));
    ARG(fpcc_pmf_to_quantized_cdf(pmf, -1, 0, nullptr, cdf));
    ARG(fpcc_rans_indexed_encode(nullptr, nullptr, 3, cdf, &start0, &len3, i32, 1, 0, b8, 64));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, 3, nullptr, &start0, &len3, i32, 1, 0, b8, 64));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, 3, cdf, nullptr, &len3, i32, 1, 0, b8, 64));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, 3, cdf, &start0, nullptr, i32, 1, 0, b8, 64));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, 3, cdf, &start0, &len3, nullptr, 1, 0, b8, 64));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, 3, cdf, &start0, &len3, i32, 1, 0, nullptr, 64));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, -1, cdf, &start0, &len3, i32, 1, 0, b8, 64));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, 3, cdf, &start0, &len3, i32, 0, 0, b8, 64));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, 3, cdf, &start0, &len3, i32, -1, 0, b8, 64));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, 3, cdf, &start0, &len3, i32, 1, 0, b8, -1));
    ARG(fpcc_rans_indexed_encode(i32, nullptr, 3, cdf, &start0, &len3, i32, 1, 1, b8, -64));
    const uint8_t stream[8] = {0, 0, 0x80, 0, 1, 2, 3, 4};
    ARG(fpcc_rans_indexed_decode(nullptr, 8, nullptr, 3, cdf, &start0, &len3, i32, 1, 0, i32));
    ARG(fpcc_rans_indexed_decode(stream, 8, nullptr, 3, nullptr, &start0, &len3, i32, 1, 0, i32));
    ARG(fpcc_rans_indexed_decode(stream, 8, nullptr, 3, cdf, nullptr, &len3, i32, 1, 0, i32));
    ARG(fpcc_rans_indexed_decode(stream, 8, nullptr, 3, cdf, &start0, nullptr, i32, 1, 0, i32));
    ARG(fpcc_rans_indexed_decode(stream, 8, nullptr, 3, cdf, &start0, &len3, nullptr, 1, 0, i32));
    ARG(fpcc_rans_indexed_decode(stream, 8, nullptr, 3, cdf, &start0, &len3, i32, 1, 0, nullptr));
    ARG(fpcc_rans_indexed_decode(stream, 8, nullptr, -1, cdf, &start0, &len3, i32, 1, 0, i32));
    ARG(fpcc_rans_indexed_decode(stream, 8, nullptr, 3, cdf, &start0, &len3, i32, 0, 0, i32));
    ARG(fpcc_rans_indexed_decode(stream, 3, nullptr, 3, cdf, &start0, &len3, i32, 1, 0, i32));
    ARG(fpcc_rans_indexed_decode(stream, 0, nullptr, 3, cdf, &start0, &len3, i32, 1, 1, i32));
    ARG(fpcc_rans_indexed_decode(stream, -8, nullptr, 3, cdf, &start0, &len3, i32, 1, 1, i32));
    ARG(fpcc_rans_binary_encode(nullptr, b16, 8, b8, 64));
    ARG(fpcc_rans_binary_encode(b8, nullptr, 8, b8, 64));
    ARG(fpcc_rans_binary_encode(b8, b16, 8, nullptr, 64));
    ARG(fpcc_rans_binary_encode(b8, b16, -1, b8, 64));
    ARG(fpcc_rans_binary_encode(b8, b16, 8, b8, -1));
    ARG(fpcc_rans_binary_encode(b8, b16, 0, b8, -100));
    ARG(fpcc_rans_binary_decode(nullptr, 8, b16, 8, b8));
    ARG(fpcc_rans_binary_decode(stream, 8, nullptr, 8, b8));
    ARG(fpcc_rans_binary_decode(stream, 8, b16, 8, nullptr));
    ARG(fpcc_rans_binary_decode(stream, 8, b16, -1, b8));
    ARG(fpcc_rans_binary_decode(stream, 3, b16, 8, b8));
    ARG(fpcc_rans_binary_decode(stream, -1, b16, 8, b8));
    ARG(fpcc_rans_binary_encode_multi(nullptr, b16, i64v, 1, b8, 64, &out64, 1));
    ARG(fpcc_rans_binary_encode_multi(b8, nullptr, i64v, 1, b8, 64, &out64, 1));
    ARG(fpcc_rans_binary_encode_multi(b8, b16, nullptr, 1, b8, 64, &out64, 1));
    ARG(fpcc_rans_binary_encode_multi(b8, b16, i64v, 1, nullptr, 64, &out64, 1));
    ARG(fpcc_rans_binary_encode_multi(b8, b16, i64v, 1, b8, 64, nullptr, 1));
    ARG(fpcc_rans_binary_encode_multi(b8, b16, i64v, -1, b8, 64, &out64, 1));
    ARG(fpcc_rans_binary_encode_multi(b8, b16, i64v, 1, b8, -64, &out64, 1));
    EXPECT_RC(fpcc_rans_binary_encode_multi(b8, b16, i64v, 1, b8, 64, &out64, -5), OK, "a negative thread count is one thread");
    REQUIRE(fpcc_simple_enc_new(15) == nullptr && fpcc_simple_enc_new(0) == nullptr && fpcc_simple_enc_new(-1) == nullptr, "an encoder of fewer than 16 bytes");
    fpcc_simple_enc_free(nullptr);
    fpcc_simple_dec_free(nullptr);
    fpcc_pool_free(nullptr);
    fpcc_simple_enc *e = fpcc_simple_enc_new(256);
    REQUIRE(e != nullptr, "no encoder");
    const int64_t rcs[] = {
        fpcc_simple_enc_push(nullptr, b16, 1, 4, b16, 1), fpcc_simple_enc_push(e, nullptr, 1, 4, b16, 1), fpcc_simple_enc_push(e, b16, 1, 4, nullptr, 1),
        fpcc_simple_enc_push(e, b16, 1, 0, b16, 1), fpcc_simple_enc_push(e, b16, 1, -4, b16, 1), fpcc_simple_enc_push(e, b16, 2, 4, b16, 3),
        fpcc_simple_enc_push(e, b16, 0, 4, b16, 3), fpcc_simple_enc_push(e, b16, -1, 4, b16, -1), fpcc_simple_enc_push(e, b16, 1, 4, b16, -1),
        fpcc_simple_enc_push_bin(nullptr, b16, 1, b8, 1), fpcc_simple_enc_push_bin(e, nullptr, 1, b8, 1), fpcc_simple_enc_push_bin(e, b16, 1, nullptr, 1),
        fpcc_simple_enc_push_bin(e, b16, 2, b8, 3), fpcc_simple_enc_push_bin(e, b16, 1, b8, -1), fpcc_simple_enc_push_bin(e, b16, -2, b8, -2),
        fpcc_simple_enc_push_ranges(nullptr, b16, b16, 1), fpcc_simple_enc_push_ranges(e, nullptr, b16, 1), fpcc_simple_enc_push_ranges(e, b16, nullptr, 1),
        fpcc_simple_enc_push_ranges(e, b16, b16, -1), fpcc_simple_enc_finish(nullptr, b8, 64), fpcc_simple_enc_finish(e, nullptr, 64),
    };
    const int64_t small = fpcc_simple_enc_finish(e, b8, -1);
    fpcc_simple_enc_free(e);
    for (size_t k = 0; k < sizeof rcs / sizeof rcs[0]; ++k) REQUIRE(rcs[k] == E_ARG, "persistent encoder, bad call %zu returned %lld", k, (long long)rcs[k]);
    EXPECT_RC(small, E_BUFFER, "finish into a negative capacity");
    REQUIRE(fpcc_simple_dec_new(nullptr, 8) == nullptr && fpcc_simple_dec_new(stream, 3) == nullptr && fpcc_simple_dec_new(stream, -1) == nullptr, "a decoder of nothing");
    fpcc_simple_dec *d = fpcc_simple_dec_new(stream, 8);
    REQUIRE(d != nullptr, "no decoder");
    const int64_t drc[] = {
        fpcc_simple_dec_pop(nullptr, b16, 1, 4, b16, 1), fpcc_simple_dec_pop(d, nullptr, 1, 4, b16, 1), fpcc_simple_dec_pop(d, b16, 1, 4, nullptr, 1),
        fpcc_simple_dec_pop(d, b16, 1, 0, b16, 1), fpcc_simple_dec_pop(d, b16, 1, -1, b16, 1), fpcc_simple_dec_pop(d, b16, 2, 4, b16, 3),
        fpcc_simple_dec_pop(d, b16, 1, 4, b16, -1), fpcc_simple_dec_pop(d, b16, -1, 4, b16, -1),
        fpcc_simple_dec_pop_bin(nullptr, b16, 1, b8, 1), fpcc_simple_dec_pop_bin(d, nullptr, 1, b8, 1), fpcc_simple_dec_pop_bin(d, b16, 1, nullptr, 1),
        fpcc_simple_dec_pop_bin(d, b16, 2, b8, 3), fpcc_simple_dec_pop_bin(d, b16, 1, b8, -1),
        fpcc_simple_dec_tell(nullptr, &state, &out64), fpcc_simple_dec_tell(d, nullptr, &out64), fpcc_simple_dec_tell(d, &state, nullptr),
    };
    fpcc_simple_dec_free(d);
    for (size_t k = 0; k < sizeof drc / sizeof drc[0]; ++k) REQUIRE(drc[k] == E_ARG, "persistent decoder, bad call %zu returned %lld", k, (long long)drc[k]);
    // the pool's entry points refuse before they touch the pool (no thread is started by this program)
    REQUIRE(fpcc_pool_new(0) == nullptr && fpcc_pool_new(-1) == nullptr && fpcc_pool_new(257) == nullptr, "a pool of no or too many threads");
    ARG(fpcc_pool_binary_encode(nullptr, &flag, 1, b8, b16, 8, b8, 64, &out64));
    ARG(fpcc_pool_histogram_encode(nullptr, &flag, 1, i32, 8, 0, i32, cdf, 3, &out64, b8, 64, &out64));
    ARG(fpcc_pool_table_decode(nullptr, stream, 8, 3, cdf, 3, 0, i32, 0, &out64));
    ARG(fpcc_pool_binary_decode(nullptr, stream, 8, b16, 8, b8, &out64));
    ARG(fpcc_pool_wait(nullptr));
    ARG(fpcc_progress_wait(nullptr, 1));
#undef ARG
    REQUIRE(std::strcmp(fpcc_host_strerror(E_ARG), "invalid argument") == 0 && fpcc_host_strerror(-99) != nullptr, "strerror");
    return "";
}

// =================================================================================================================================
// hostile decoder input: every decoder returns, whatever it is given (what it decodes is unspecified)
// =================================================================================================================================
struct Hostile {
    std::string name;
    int64_t valid_n;                                                  // symbols of the valid stream
    std::function<Bytes()> valid;                                     // a valid stream of about 200 bytes
    std::function<int64_t(const Exact<uint8_t> &, int64_t n)> decode;          // decodes n symbols from an exact heap copy
};

std::string run_hostile(const Hostile &h) {
    Rng rng(112);
    const Bytes valid = h.valid();
    const int64_t L = static_cast<int64_t>(valid.size());
    REQUIRE(L >= 100 && L <= 400, "%s: the valid stream has %lld bytes", h.name.c_str(), (long long)L);
    {
        Exact<uint8_t> s(valid);
        EXPECT_RC(h.decode(s, h.valid_n), OK, "%s: the valid stream", h.name.c_str());
    }
    for (int64_t len = 4; len < L; ++len) {                           // truncated at every length; asked for all symbols and for more
        Exact<uint8_t> s(valid.data(), len);
        (void)h.decode(s, h.valid_n);
        if (len % 16 == 0) (void)h.decode(s, 3 * h.valid_n);
    }
    for (int64_t len : {int64_t(4), int64_t(5), int64_t(6), int64_t(64), L}) {
        Exact<uint8_t> s(Bytes(static_cast<size_t>(len), 0xff));
        (void)h.decode(s, h.valid_n);
    }
    for (int k = 0; k < 40; ++k) {                                    // random bytes behind a valid first state
        Bytes b(static_cast<size_t>(4 + rng() % 300));
        for (auto &v : b) v = static_cast<uint8_t>(rng());
        const uint32_t first = (1u << 23) + static_cast<uint32_t>(rng() % ((1u << 31) - (1u << 23)));
        for (int j = 0; j < 4; ++j) b[j] = static_cast<uint8_t>(first >> (8 * j));
        if (k % 4 == 0) std::fill(b.begin() + 4, b.end(), static_cast<uint8_t>(0));
        Exact<uint8_t> s(b);
        (void)h.decode(s, h.valid_n);
        (void)h.decode(s, 5 * h.valid_n);
    }
    for (uint32_t first : {0u, 1u, 127u, 128u, (1u << 23) - 1u}) {    // a first state below 2^23 is no stream: refused
        Bytes b = valid;
        for (int j = 0; j < 4; ++j) b[j] = static_cast<uint8_t>(first >> (8 * j));
        Exact<uint8_t> s(b);
        const int64_t rc = h.decode(s, h.valid_n);
        REQUIRE(rc == E_ARG, "%s: a first state of %u returned %lld", h.name.c_str(), first, (long long)rc);
    }
    for (uint32_t first : {0x7fffffffu, 0x80000000u, 0xffffffffu, 1u << 23}) {          // first states at and past the upper end
        Bytes b = valid;
        for (int j = 0; j < 4; ++j) b[j] = static_cast<uint8_t>(first >> (8 * j));
        Exact<uint8_t> s(b);
        (void)h.decode(s, h.valid_n);
    }
    return "";
}

std::string check_hostile_decoders() {
    Rng rng(113);
    std::vector<Hostile> hs;
    for (int overflow : {0, 1})
        for (int n_tables : {1, 3}) {
            std::vector<std::vector<uint32_t>> rows;
            std::vector<int32_t> off;
            for (int t = 0; t < n_tables; ++t) { rows.push_back(rand_cdf(rng, 3 + 5 * t)); off.push_back(t == 1 ? INT32_MAX - 20 : -t); }
            const Tab tab = make_tab(rows, off);
            const int64_t n = overflow ? 120 : 600;
            std::vector<int32_t> sym(static_cast<size_t>(n));
            for (int64_t i = 0; i < n; ++i) {
                const int64_t ti = i % n_tables;
                const int bins = static_cast<int>(tab.len[ti]) - 1 - overflow;
                sym[i] = off[ti] + static_cast<int32_t>(rng() % static_cast<uint64_t>(bins));
                if (overflow && i % 3 == 0) sym[i] = off[ti] - static_cast<int32_t>(rng() % 100000);
            }
            hs.push_back({fmt("indexed, overflow %d, %d tables", overflow, n_tables), n,
                          [=] { Bytes s; lib_idx_enc(tab, sym, nullptr, overflow, 40 * n + 64, s); return s; },
                          [=](const Exact<uint8_t> &s, int64_t m) {
                              Exact<int32_t> out(m), o(tab.off);
                              Exact<uint32_t> c(tab.flat);
                              Exact<int64_t> st(tab.start), ln(tab.len);
                              return fpcc_rans_indexed_decode(s.p, s.n, nullptr, m, c.p, st.p, ln.p, o.p, tab.count(), overflow, out.p);
                          }});
        }
    {   // the lookup-table decoder (one table, >= 8192 symbols): a peaked table keeps the valid stream short
        const Tab tab = make_tab({{0, 65000, 65200, 65535, 65536}}, {-1});
        const int64_t n = 20000;
        std::vector<int32_t> sym(static_cast<size_t>(n));
        for (auto &s : sym) { const uint32_t r = static_cast<uint32_t>(rng() % 65536); s = -1 + (r >= 65535 ? 3 : r >= 65200 ? 2 : r >= 65000 ? 1 : 0); }
        hs.push_back({"indexed, lookup table", n, [=] { Bytes s; lib_idx_enc(tab, sym, nullptr, 0, 4 * n + 64, s); return s; },
                      [=](const Exact<uint8_t> &s, int64_t m) {
                          Exact<int32_t> out(m), o(tab.off);
                          Exact<uint32_t> c(tab.flat);
                          Exact<int64_t> st(tab.start), ln(tab.len);
                          return fpcc_rans_indexed_decode(s.p, s.n, nullptr, m, c.p, st.p, ln.p, o.p, 1, 0, out.p);
                      }});
    }
    {
        std::vector<uint8_t> bits;
        std::vector<uint16_t> prob;
        rand_binary(rng, 1500, bits, prob);
        hs.push_back({"binary", 1500, [=] { Bytes s; lib_bin_enc(bits, prob, 4 * 1500 + 64, s); return s; },
                      [=](const Exact<uint8_t> &s, int64_t m) {
                          std::vector<uint16_t> p(static_cast<size_t>(m));
                          for (int64_t i = 0; i < m; ++i) p[i] = i % 97 == 5 ? 0 : prob[i % 1500];      // (a zero probability among them: the decoder takes any)
                          Exact<uint16_t> pp(p);
                          Exact<uint8_t> out(m);
                          return fpcc_rans_binary_decode(s.p, s.n, pp.p, m, out.p);
                      }});
    }
    for (int64_t width : {7, 40, 255}) {
        const int64_t n = 260;
        const Block b = rows_block(rng, n, width, false, Block::ROWS);
        hs.push_back({fmt("persistent, width %lld", (long long)width), n, [=] { return orc_simple_stream({b}, 1 << 16); },
                      [=](const Exact<uint8_t> &s, int64_t m) -> int64_t {
                          fpcc_simple_dec *d = fpcc_simple_dec_new(s.p, s.n);
                          if (!d) return E_ARG;
                          std::vector<uint16_t> rows(static_cast<size_t>(m * width));
                          for (int64_t i = 0; i < m; ++i) std::copy_n(b.rows.data() + (i % n) * width, width, rows.data() + i * width);
                          if (m > n) for (int64_t j = 0; j < width; ++j) rows[static_cast<size_t>(n * width + j)] = static_cast<uint16_t>(40000 - 3 * j);      // a decreasing row
                          Exact<uint16_t> r(rows), out(m);
                          int64_t rc = fpcc_simple_dec_pop(d, r.p, m, width, out.p, m);
                          for (int64_t i = 0; i < m && rc == OK; ++i) if (out.p[i] >= width) rc = -100;          // whatever is decoded is a symbol of the row
                          uint32_t state;
                          int64_t pos;
                          if (rc == OK) rc = fpcc_simple_dec_tell(d, &state, &pos);
                          fpcc_simple_dec_free(d);
                          return rc;
                      }});
    }
    {
        const Block b = bin_block(rng, 1500, false);
        hs.push_back({"persistent, binary", 1500, [=] { return orc_simple_stream({b}, 1 << 16); },
                      [=](const Exact<uint8_t> &s, int64_t m) -> int64_t {
                          fpcc_simple_dec *d = fpcc_simple_dec_new(s.p, s.n);
                          if (!d) return E_ARG;
                          std::vector<uint16_t> edge(static_cast<size_t>(m));
                          for (int64_t i = 0; i < m; ++i) edge[i] = i >= 1500 && i % 5 == 0 ? 0 : b.rows[i % 1500];
                          Exact<uint16_t> e(edge);
                          Exact<uint8_t> out(m);
                          const int64_t rc = fpcc_simple_dec_pop_bin(d, e.p, m, out.p, m);
                          fpcc_simple_dec_free(d);
                          return rc;
                      }});
    }
    for (const Hostile &h : hs) PROPAGATE(run_hostile(h));
    return "";
}

// =================================================================================================================================
struct Check { const char *name; std::string (*fn)(); };
const Check kChecks[] = {
    {"golden_replay", check_golden_replay},
    {"binary_differential", check_binary_differential},
    {"binary_multi", check_binary_multi},
    {"indexed_differential", check_indexed_differential},
    {"indexed_single_table", check_indexed_single_table},
    {"escape_values", check_escape_values},
    {"simple_differential", check_simple_differential},
    {"pmf_differential", check_pmf_differential},
    {"exact_fit", check_exact_fit},
    {"err_binary_zero_probability", check_err_binary_zero_probability},
    {"err_multi_start", check_err_multi_start},
    {"err_simple_push", check_err_simple_push},
    {"err_push_ranges", check_err_push_ranges},
    {"err_indexed_symbols", check_err_indexed_symbols},
    {"err_indexed_short_tables", check_err_indexed_short_tables},
    {"err_indexed_malformed_tables", check_err_indexed_malformed_tables},
    {"err_null_and_negative", check_err_null_and_negative},
    {"hostile_decoders", check_hostile_decoders},
};

// ns per symbol of the two encoders on the serial tail of a frame, 11 runs each
int time_mode() {
    const int64_t n = 709000;
    Rng rng(7);
    std::vector<uint8_t> bits;
    std::vector<uint16_t> prob;
    rand_binary(rng, n, bits, prob);
    std::vector<uint16_t> start(static_cast<size_t>(n)), fm1(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) {
        start[i] = static_cast<uint16_t>(rng() % 65000);
        const uint32_t room = 65536u - start[i];
        fm1[i] = static_cast<uint16_t>(rng() % 2 ? rng() % std::min<uint32_t>(room, 64u) : rng() % room);
    }
    Bytes out(static_cast<size_t>(4 * n + 64));
    fpcc_simple_enc *e = fpcc_simple_enc_new(4 * n + 64);
    if (!e) return 1;
    auto report = [&](const char *name, std::vector<double> ns) {
        std::printf("time %s runs", name);
        for (double v : ns) std::printf(" %.3f", v);
        std::sort(ns.begin(), ns.end());
        std::printf("\ntime %s ns_per_symbol median %.3f min %.3f max %.3f\n", name, ns[ns.size() / 2], ns.front(), ns.back());
    };
    std::vector<double> a, b;
    int64_t sink = 0;
    for (int run = -2; run < 11; ++run) {                              // two warm-up runs
        auto t0 = std::chrono::steady_clock::now();
        sink += fpcc_rans_binary_encode(bits.data(), prob.data(), n, out.data(), static_cast<int64_t>(out.size()));
        auto t1 = std::chrono::steady_clock::now();
        sink += fpcc_simple_enc_push_ranges(e, start.data(), fm1.data(), n);
        auto t2 = std::chrono::steady_clock::now();
        sink += fpcc_simple_enc_finish(e, out.data(), static_cast<int64_t>(out.size()));
        if (run < 0) continue;
        a.push_back(std::chrono::duration<double, std::nano>(t1 - t0).count() / n);
        b.push_back(std::chrono::duration<double, std::nano>(t2 - t1).count() / n);
    }
    fpcc_simple_enc_free(e);
    report("fpcc_rans_binary_encode", a);
    report("fpcc_simple_enc_push_ranges", b);
    std::printf("time checksum %lld\n", (long long)sink);
    return sink > 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    std::string only;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--time") return time_mode();
        if (a == "--list") { for (const Check &c : kChecks) std::printf("%s\n", c.name); return 0; }
        if (a == "--only" && i + 1 < argc) only = argv[++i];
        else g_golden_path = a;
    }
    int failed = 0, ran = 0;
    for (const Check &c : kChecks) {
        if (!only.empty() && std::string(c.name).find(only) == std::string::npos) continue;
        if (std::string(c.name) == "golden_replay" && g_golden_path.empty()) { std::printf("golden_replay: FAIL no golden file given\n"); ++failed; ++ran; continue; }
        const std::string msg = c.fn();
        ++ran;
        if (msg.empty()) std::printf("%s: ok\n", c.name);
        else { std::printf("%s: FAIL %s\n", c.name, msg.c_str()); ++failed; }
    }
    for (const auto &kv : g_replayed) std::printf("replayed %s %d\n", kv.first.c_str(), kv.second);
    if (!g_escape_note.empty()) std::printf("note escape_values: %s\n", g_escape_note.c_str());
    std::printf("coder_checks: %d checks, %d failed\n", ran, failed);
    return failed || !ran ? 1 : 0;
}
