// Stand-alone checks of the threaded parts of libfpcc_host (fastpcc_amd/csrc/host/rans_host.cpp) for the sanitizer builds of
// tests/test_host_sanitized.py: the background coder pool and the row warmers of the 255-ary decoder.  Own main, linked with the
// library's source and the plain-C test oracle oracle/rans.c; built once under AddressSanitizer + UBSan and once under
// ThreadSanitizer.  The hand-over pattern is that of tools/r05/pool_stress.cpp and warmers_stress.cpp, scaled to seconds.
//
//   pool_checks [frames per context = 40]        every check prints `name: ok` or `name: FAIL ...`; exit status 1 if any failed
//
// The row warmers read FPCC_HOST_WARMERS once per process: the Python test runs this program with 0, 1 and 4 helpers.
#include "../../include/fpcc_host.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

extern "C" {
int64_t orc_binary_encode(const uint8_t *bits, const uint32_t *prob1, int64_t n, uint8_t *out, int64_t cap);
struct orc_simple_enc;
struct orc_simple_dec;
orc_simple_enc *orc_simple_enc_new(int64_t cap);
void orc_simple_enc_free(orc_simple_enc *s);
int64_t orc_simple_enc_push(orc_simple_enc *s, const uint16_t *rows, int64_t n_rows, int64_t width, const uint16_t *sym, int64_t n);
int64_t orc_simple_enc_finish(orc_simple_enc *s, uint8_t *out, int64_t out_cap);
orc_simple_dec *orc_simple_dec_new(const uint8_t *bytes);
void orc_simple_dec_free(orc_simple_dec *s);
void orc_simple_dec_pop(orc_simple_dec *s, const uint16_t *rows, int64_t n_rows, int64_t width, uint16_t *sym_out, int64_t n);
}

namespace {

using Rng = std::mt19937_64;

struct Level {
    std::vector<uint8_t> bits, want_bits, out;
    std::vector<uint16_t> prob, want_prob;
    int64_t len = 0;
};

// One context: its own pool, producer and consumer, `frames` frames.  Returns "" or what went wrong.
std::string run_context(int ctx, int frames) {
    Rng rng(1234 + ctx);
    fpcc_pool *pool = fpcc_pool_new(4);
    if (!pool) return "no pool";
    std::string bad;
    auto fail = [&](int frame, const std::string &what) { bad = "context " + std::to_string(ctx) + ", frame " + std::to_string(frame) + ": " + what; };
    for (int f = 0; f < frames && bad.empty(); ++f) {
        // every buffer of a frame lives in this scope: freed at its end, after the waits
        std::vector<uint32_t> flags(16, 0);
        const int n_levels = 6;
        std::vector<Level> lv(n_levels);
        for (int l = 0; l < n_levels; ++l) {
            const int64_t n = 8 + static_cast<int64_t>(rng() % (l == n_levels - 1 ? 20000 : 3000));
            Level &L = lv[l];
            L.want_bits.resize(n);
            L.want_prob.resize(n);
            for (int64_t i = 0; i < n; ++i) {
                L.want_prob[i] = static_cast<uint16_t>(1 + rng() % 65535);
                L.want_bits[i] = (rng() & 0xffff) < L.want_prob[i];
            }
            // what the job must NOT read: poison (a probability of 0 makes the coder refuse, a wrong bit makes the round trip fail)
            L.bits.assign(n, 1);
            L.prob.assign(n, 0);
            L.out.resize(l % 2 ? 2 * n + 8 : 2 * n + 7);                   // both steps of the binary encoder
        }
        const int64_t n_sym = 64 + static_cast<int64_t>(rng() % 30000);
        std::vector<int32_t> want_sym(n_sym), sym(n_sym, 1 << 20);
        for (auto &s : want_sym) s = static_cast<int32_t>(rng() % 41) - 20;
        std::vector<uint8_t> sym_out(4 * n_sym + 64);
        std::vector<uint32_t> cdf(64);
        int64_t cdf_len = 0, sym_len = 0;
        int32_t offset = 0;
        // submit first, on buffers that still hold poison ...
        int n_flags = 0;
        if (fpcc_pool_histogram_encode(pool, &flags[n_flags], 1, sym.data(), n_sym, 0, &offset, cdf.data(), static_cast<int64_t>(cdf.size()), &cdf_len,
                                       sym_out.data(), static_cast<int64_t>(sym_out.size()), &sym_len) < 0) fail(f, "histogram job refused");
        const int sym_flag = n_flags++;
        std::vector<int> level_flag(n_levels);
        for (int l = n_levels - 1; l >= 0 && bad.empty(); --l) {
            Level &L = lv[l];
            level_flag[l] = n_flags;
            if (fpcc_pool_binary_encode(pool, &flags[n_flags++], 1, L.bits.data(), L.prob.data(), static_cast<int64_t>(L.bits.size()), L.out.data(),
                                        static_cast<int64_t>(L.out.size()), &L.len) < 0) fail(f, "binary job refused");
        }
        // ... then the producer delivers the inputs, each job's flag last
        std::thread producer([&] {
            Rng prng(99 + ctx * 1000 + f);
            auto deliver = [&](void *dst, const void *src, size_t bytes, uint32_t *flag) {
                if (prng() % 4 == 0) std::this_thread::sleep_for(std::chrono::microseconds(prng() % 200));
                std::memcpy(dst, src, bytes);
                if (flag) __atomic_store_n(flag, 1u, __ATOMIC_RELEASE);
            };
            deliver(sym.data(), want_sym.data(), n_sym * sizeof(int32_t), &flags[sym_flag]);
            for (int l = n_levels - 1; l >= 0; --l) {
                deliver(lv[l].bits.data(), lv[l].want_bits.data(), lv[l].bits.size(), nullptr);
                deliver(lv[l].prob.data(), lv[l].want_prob.data(), lv[l].prob.size() * 2, &flags[level_flag[l]]);
            }
        });
        const int64_t rc = fpcc_pool_wait(pool);
        producer.join();
        if (rc < 0) { fail(f, std::string("pool wait: ") + fpcc_host_strerror(rc)); break; }
        // every stream is the oracle's and decodes to what was delivered
        for (int l = 0; l < n_levels && bad.empty(); ++l) {
            Level &L = lv[l];
            const int64_t n = static_cast<int64_t>(L.bits.size());
            std::vector<uint32_t> p32(L.want_prob.begin(), L.want_prob.end());
            std::vector<uint8_t> want(2 * n + 64), got(n);
            const int64_t want_len = orc_binary_encode(L.want_bits.data(), p32.data(), n, want.data(), static_cast<int64_t>(want.size()));
            if (L.len != want_len || std::memcmp(L.out.data() + L.out.size() - L.len, want.data() + want.size() - want_len, want_len) != 0)
                fail(f, "level " + std::to_string(l) + ": not the oracle's stream");
            else if (fpcc_rans_binary_decode(L.out.data() + L.out.size() - L.len, L.len, L.want_prob.data(), n, got.data()) < 0 || got != L.want_bits)
                fail(f, "level " + std::to_string(l) + ": round trip differs");
        }
        // decoder side: one table decode consumed by prefixes while three binary decodes run beside it
        if (bad.empty()) {
            std::vector<int32_t> dec(n_sym, -99);
            int64_t progress = 0, done[3] = {0, 0, 0};
            std::vector<std::vector<uint8_t>> bits(3);
            if (sym_len < 4 || fpcc_pool_table_decode(pool, sym_out.data() + sym_out.size() - sym_len, sym_len, n_sym, cdf.data(), cdf_len, offset, dec.data(), 16,
                                                      &progress) < 0) fail(f, "table decode refused");
            for (int k = 0; k < 3 && bad.empty(); ++k) {
                Level &L = lv[n_levels - 1 - k];
                bits[k].assign(L.bits.size(), 7);
                if (fpcc_pool_binary_decode(pool, L.out.data() + L.out.size() - L.len, L.len, L.want_prob.data(), static_cast<int64_t>(L.bits.size()), bits[k].data(),
                                            &done[k]) < 0) fail(f, "binary decode refused");
            }
            int64_t taken = 0;
            while (bad.empty() && taken < n_sym) {
                const int64_t want = std::min<int64_t>(n_sym, taken + 1 + static_cast<int64_t>(rng() % 9000));
                if (fpcc_progress_wait(&progress, want) < 0) { fail(f, "progress wait"); break; }
                if (std::memcmp(dec.data() + taken, want_sym.data() + taken, (want - taken) * sizeof(int32_t)) != 0) fail(f, "decoded prefix differs");
                taken = want;
            }
            for (int k = 0; k < 3 && bad.empty(); ++k) {
                if (fpcc_progress_wait(&done[k], 1) != 1) fail(f, "binary decode job " + std::to_string(k));
                else if (bits[k] != lv[n_levels - 1 - k].want_bits) fail(f, "binary decode job " + std::to_string(k) + " differs");
            }
            if (fpcc_pool_wait(pool) < 0 && bad.empty()) fail(f, "pool wait after the decodes");
        }
        // one job with a zero probability among valid ones: reported once, and the pool goes on
        if (bad.empty() && f % 8 == 3) {
            Level &L = lv[f % n_levels];
            std::vector<uint16_t> zero = L.want_prob;
            zero[zero.size() / 2] = 0;
            int64_t len_bad = 0, len_ok = 0;
            std::vector<uint8_t> out_bad(L.out.size()), out_ok(L.out.size());
            const int64_t n = static_cast<int64_t>(L.bits.size());
            if (fpcc_pool_binary_encode(pool, nullptr, 0, L.want_bits.data(), zero.data(), n, out_bad.data(), static_cast<int64_t>(out_bad.size()), &len_bad) < 0 ||
                fpcc_pool_binary_encode(pool, nullptr, 0, L.want_bits.data(), L.want_prob.data(), n, out_ok.data(), static_cast<int64_t>(out_ok.size()), &len_ok) < 0)
                fail(f, "jobs refused");
            const int64_t first = fpcc_pool_wait(pool), second = fpcc_pool_wait(pool);
            if (first != FPCC_HOST_E_ARG || second != FPCC_HOST_OK || len_bad != FPCC_HOST_E_ARG || len_ok != L.len ||
                std::memcmp(out_ok.data() + out_ok.size() - len_ok, L.out.data() + L.out.size() - L.len, L.len) != 0)
                fail(f, "zero probability: waits returned " + std::to_string(first) + ", " + std::to_string(second) + ", lengths " + std::to_string(len_bad) + ", " +
                            std::to_string(len_ok));
        }
    }
    fpcc_pool_free(pool);
    return bad;
}

std::string check_pool(int frames) {
    std::string msg[2];
    std::thread other([&] { msg[1] = run_context(1, frames); });
    msg[0] = run_context(0, frames);
    other.join();
    return msg[0].empty() ? msg[1] : msg[0];
}

// ---- row warmers ----------------------------------------------------------------------------------------------------------------
// `n` rows of width 255, one per symbol, in a heap block that is freed the moment fpcc_simple_dec_pop returns: a helper that still
// reads it then is a use after free.  The symbols must be the oracle decoder's.
std::string warm_round(int seed, int64_t n) {
    Rng rng(seed);
    const int64_t width = 255;
    std::unique_ptr<uint16_t[]> rows(new uint16_t[static_cast<size_t>(n * width)]);
    std::vector<uint16_t> sym(static_cast<size_t>(n)), out(static_cast<size_t>(n)), oout(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) {
        uint32_t acc = 0;
        for (int64_t j = 0; j < width; ++j) { acc += 1 + static_cast<uint32_t>(rng() % 250); rows[static_cast<size_t>(i * width + j)] = static_cast<uint16_t>(acc); }
        rows[static_cast<size_t>(i * width + width - 1)] = 65535;
        sym[static_cast<size_t>(i)] = static_cast<uint16_t>(rng() % width);
    }
    const int64_t cap = 2 * n + 64;
    std::vector<uint8_t> stream(static_cast<size_t>(cap)), want(static_cast<size_t>(cap));
    fpcc_simple_enc *e = fpcc_simple_enc_new(cap);
    if (!e || fpcc_simple_enc_push(e, rows.get(), n, width, sym.data(), n) < 0) { fpcc_simple_enc_free(e); return "encode failed"; }
    const int64_t len = fpcc_simple_enc_finish(e, stream.data(), cap);
    fpcc_simple_enc_free(e);
    orc_simple_enc *oe = orc_simple_enc_new(cap);
    orc_simple_enc_push(oe, rows.get(), n, width, sym.data(), n);
    const int64_t want_len = orc_simple_enc_finish(oe, want.data(), cap);
    orc_simple_enc_free(oe);
    if (len < 4 || len != want_len || std::memcmp(stream.data(), want.data(), static_cast<size_t>(len)) != 0) return "not the oracle's stream";
    orc_simple_dec *od = orc_simple_dec_new(stream.data());
    orc_simple_dec_pop(od, rows.get(), n, width, oout.data(), n);
    orc_simple_dec_free(od);
    fpcc_simple_dec *d = fpcc_simple_dec_new(stream.data(), len);
    if (!d) return "no decoder";
    const int64_t rc = fpcc_simple_dec_pop(d, rows.get(), n, width, out.data(), n);
    rows.reset();                                          // freed right after the decode
    fpcc_simple_dec_free(d);
    if (rc < 0) return "decode failed";
    if (out != oout || out != sym) return "symbols differ from the oracle decoder's";
    return "";
}

std::string check_warmers_one_thread() {
    // the helpers start at 2048 rows AND 1 MiB of rows: 2048 x 510 B is just under that, 2100 rows are over it
    for (int64_t n : {2047, 2048, 2100, 4200}) {
        const std::string m = warm_round(static_cast<int>(n), n);
        if (!m.empty()) return std::to_string(n) + " rows: " + m;
    }
    return "";
}

std::string check_warmers_two_threads() {
    std::string msg[2];
    auto work = [&](int t) {
        for (int r = 0; r < 3 && msg[t].empty(); ++r) msg[t] = warm_round(100 * t + r, r == 1 ? 2100 : 4200);
    };
    std::thread other(work, 1);
    work(0);
    other.join();
    return msg[0].empty() ? msg[1] : msg[0];
}

}  // namespace

int main(int argc, char **argv) {
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    const int frames = argc > 1 ? std::atoi(argv[1]) : 40;
    const char *warmers = std::getenv("FPCC_HOST_WARMERS");
    std::printf("pool_checks: %d frames per context, FPCC_HOST_WARMERS=%s\n", frames, warmers ? warmers : "(unset)");
    int failed = 0;
    auto report = [&](const char *name, const std::string &msg) {
        if (msg.empty()) std::printf("%s: ok\n", name);
        else { std::printf("%s: FAIL %s\n", name, msg.c_str()); ++failed; }
    };
    report("pool_two_contexts", check_pool(frames));
    report("warmers_one_thread", check_warmers_one_thread());
    report("warmers_two_threads", check_warmers_two_threads());
    std::printf("pool_checks: 3 checks, %d failed\n", failed);
    return failed ? 1 : 0;
}
