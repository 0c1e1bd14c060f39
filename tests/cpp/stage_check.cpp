// Drives the staging bookkeeping of the matcher's host forms (orb_slam2_comment_amd/csrc/orbhip_stage.h) against plain
// malloc'ed buffers that stand in for the pinned and the device image, for test_stage_cpu.py: argv[1] names the case
// (sizes, fillers, outputs, capacity).  Exit code 0 and "ok" when every check of the case holds; each failed check
// prints its line.  Every buffer has exactly the size the bookkeeping asks for, so that a sanitizer build sees any
// byte written or read past it.
#include "orbhip_stage.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using orbhip::Stage;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

struct V12 { float x, y, z; };
static_assert(sizeof(V12) == 12, "a 12-byte element");

// both passes of a description, as stage_send makes them: measure, then run on buffers of exactly that size
struct Images {
    uint8_t *h, *d;
    size_t total;
    Stage st;
    template <class F> explicit Images(F &&pieces)
    {
        total = orbhip::stage_measure(pieces);
        h = (uint8_t *)malloc(total ? total : 1);
        d = (uint8_t *)malloc(total ? total : 1);
        memset(h, 0xEE, total);
        memset(d, 0xDD, total);
        st.h = h; st.d = d;
        pieces(st);
    }
    ~Images() { free(h); free(d); }
    void send() { memcpy(d, h, st.off); }   // the one host-to-device copy
    // the one device-to-host copy, into a buffer of exactly the span, then the scatter
    void fetch()
    {
        const size_t b = st.out_begin(), n = st.out_end() - b;
        std::vector<uint8_t> span(d + b, d + b + n);
        st.scatter(span.data());
        st.img = nullptr;   // the vector goes away
    }
    size_t at(const void *dev) const { return (size_t)((const uint8_t *)dev - d); }
};

static const size_t kCounts[] = {0, 1, 255, 256, 257};

static void sizes()
{
    std::vector<uint8_t> src(257, 7);
    const V12 v[3] = {{1, 2, 3}, {4, 5, 6}, {7, 8, 9}};
    const uint8_t *dev[5];
    const V12 *dv;
    const uint8_t *tail;
    Images I([&](Stage &st) {
        for (int i = 0; i < 5; ++i) dev[i] = st.put(src.data(), kCounts[i]);
        dv = st.put(v, 3);
        tail = st.room<uint8_t>(1);
    });
    // 0 | 1 -> 256 | 255 -> 256 | 256 -> 256 | 257 -> 512 | 36 -> 256 | 1 -> 256
    CHECK(I.total == 1792 && I.st.off == I.total);
    const size_t want[5] = {0, 0, 256, 512, 768};
    for (int i = 0; i < 5; ++i) CHECK(I.at(dev[i]) == want[i] && I.at(dev[i]) % 256 == 0);
    CHECK(dev[0] == dev[1]);                       // the empty piece takes no room and yields the next piece's address
    CHECK(I.at(dv) == 1280 && I.at(tail) == 1536);
    CHECK(!memcmp(I.h + 1280, v, 36) && I.h[1280 + 36] == 0xEE);
    for (int i = 1; i < 5; ++i) {
        CHECK(!memcmp(I.h + want[i], src.data(), kCounts[i]));
        if (kCounts[i] % 256) CHECK(I.h[want[i] + kCounts[i]] == 0xEE);   // put copies count elements, no more
    }
    CHECK(orbhip::al256(0) == 0 && orbhip::al256(1) == 256 && orbhip::al256(256) == 256 && orbhip::al256(257) == 512);
}

static void fillers()
{
    int calls[6] = {0, 0, 0, 0, 0, 0}, passes = 0;
    uint8_t *seen[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint8_t *dev[6];
    bool measuring_called = false;
    auto pieces = [&](Stage &st) {
        ++passes;
        for (int i = 0; i < 5; ++i)
            dev[i] = st.fill<uint8_t>(kCounts[i], [&, i](uint8_t *host) {
                ++calls[i]; seen[i] = host;
                if (!st.h) measuring_called = true;
                memset(host, 0x10 + i, kCounts[i]);
            });
        dev[5] = (uint8_t *)st.fill<V12>(3, [&](V12 *host) { ++calls[5]; seen[5] = (uint8_t *)host; host[2].z = 9.f; });
    };
    Images I(pieces);
    CHECK(passes == 2 && !measuring_called);
    CHECK(calls[0] == 0);                          // never for an empty piece
    for (int i = 1; i < 6; ++i) {
        CHECK(calls[i] == 1);                      // once, in the real pass
        CHECK(seen[i] == I.h + I.at(dev[i]));      // with the host address of the same bytes
    }
    for (int i = 1; i < 5; ++i) CHECK(I.h[I.at(dev[i])] == 0x10 + i && I.h[I.at(dev[i]) + kCounts[i] - 1] == 0x10 + i);
    CHECK(I.total == 1536 && I.st.off == I.total);

    // several pieces filled by one sweep: the sweep runs once, in the real pass only, and host() is the piece's host address
    int sweeps = 0;
    const V12 *dv;
    const uint8_t *db;
    Images S([&](Stage &st) {
        dv = st.room<V12>(3);
        db = st.room<uint8_t>(257);
        st.sweep([&] {
            ++sweeps;
            CHECK(st.h != nullptr);
            for (int r = 0; r < 3; ++r) { st.host(dv)[r].x = (float)r; st.host(db)[r * 128] = (uint8_t)(0x20 + r); }
        });
    });
    CHECK(sweeps == 1 && S.total == 768);
    CHECK((uint8_t *)S.st.host(dv) == S.h && S.st.host(db) == S.h + 256);
    CHECK(((const V12 *)S.h)[2].x == 2.f && S.h[256] == 0x20 && S.h[256 + 256] == 0x22 && S.h[256 + 255] == 0xEE);
}

// a host array between guard bytes
struct Guarded {
    std::vector<uint8_t> b;
    size_t n;
    explicit Guarded(size_t bytes, uint8_t fill) : b(bytes + 32, 0xA5), n(bytes) { memset(data(), fill, bytes); }
    uint8_t *data() { return b.data() + 16; }
    bool guards() const
    {
        for (size_t i = 0; i < 16; ++i) if (b[i] != 0xA5 || b[16 + n + i] != 0xA5) return false;
        return true;
    }
    bool all(uint8_t v) const { for (size_t i = 0; i < n; ++i) if (b[16 + i] != v) return false; return true; }
};

static void outputs()
{
    Guarded a(257, 1), skipped(40, 3), c(36, 4), e(5, 5);
    std::vector<uint8_t> in(300, 9), mid(100, 8);
    const uint8_t *d_in, *d_mid, *d_skip;   // inputs: put hands out read-only device addresses
    uint8_t *d_a, *d_c, *d_e, *d_span;
    const bool want_skipped = false;
    Images I([&](Stage &st) {
        d_in = st.put(in.data(), in.size());
        d_a = st.inout(a.data(), a.n);                                   // staged from the host, travels back
        d_mid = st.put(mid.data(), mid.size());                          // a plain piece between two outputs
        d_skip = want_skipped ? st.inout(skipped.data(), skipped.n) : st.put(skipped.data(), skipped.n);
        d_c = (uint8_t *)st.out((V12 *)c.data(), 3);                     // output only
        d_span = st.out((uint8_t *)nullptr, 7);                          // part of the span, fetched through image()
        d_e = st.fill<uint8_t>(e.n, [&](uint8_t *h) { memset(h, 6, e.n); });
        st.back(e.data(), d_e, e.n);                                     // filled in place and recorded
        st.out(e.data(), 0);                                             // an empty output is not recorded
    });
    CHECK(I.st.n_out == 4 && !I.st.out_overflow);
    CHECK(I.st.out_begin() == I.at(d_a) && I.st.out_end() == I.at(d_e) + e.n);   // first output .. end of the last
    CHECK(I.st.out_begin() == 512 && I.st.out_end() == 512 + 512 + 256 + 256 + 256 + 256 + 5);
    CHECK(!memcmp(I.h + I.at(d_a), a.data(), a.n) && !memcmp(I.h + I.at(d_skip), skipped.data(), skipped.n));
    I.send();
    CHECK(!memcmp(I.d, I.h, I.total));
    // the kernels: every byte of the span changes, padding and the plain pieces included
    for (size_t i = I.st.out_begin(); i < I.total; ++i) I.d[i] = (uint8_t)(0x40 + (i >> 8));
    {
        const size_t b = I.st.out_begin(), n = I.st.out_end() - b;
        std::vector<uint8_t> span(I.d + b, I.d + b + n);
        I.st.scatter(span.data());
        CHECK(I.st.image(d_span) == span.data() + (I.at(d_span) - b) && I.st.image(d_span)[6] == (uint8_t)(0x40 + (I.at(d_span) >> 8)));
        CHECK(I.st.image((const V12 *)d_c) == (const V12 *)(span.data() + (I.at(d_c) - b)));
    }
    // the 257 bytes of a: exactly these, across a 256-byte line
    for (size_t i = 0; i < a.n; ++i) CHECK(a.data()[i] == (uint8_t)(0x40 + ((512 + i) >> 8)));
    CHECK(c.all((uint8_t)(0x40 + (I.at(d_c) >> 8))) && e.all((uint8_t)(0x40 + (I.at(d_e) >> 8))));
    CHECK(skipped.all(3));                                                  // the skipped optional output is not touched
    CHECK(a.guards() && skipped.guards() && c.guards() && e.guards());
    for (size_t i = 0; i < in.size(); ++i) CHECK(in[i] == 9);
    for (size_t i = 0; i < mid.size(); ++i) CHECK(mid[i] == 8);
    (void)d_in; (void)d_mid;

    // no output at all: an empty span at the end of the image, and a scatter that touches nothing
    Images N([&](Stage &st) { st.put(in.data(), 10); });
    CHECK(N.st.n_out == 0 && N.st.out_begin() == N.st.off && N.st.out_end() == N.st.off);
    N.fetch();
}

static void capacity()
{
    std::vector<Guarded> hosts;
    for (int i = 0; i <= Stage::kMaxOut; ++i) hosts.emplace_back(4, (uint8_t)i);
    for (int extra = 0; extra <= 1; ++extra) {
        const int n = Stage::kMaxOut + extra;
        bool measured_overflow = false;
        auto pieces = [&](Stage &st) { for (int i = 0; i < n; ++i) st.inout(hosts[i].data(), 4); };
        orbhip::stage_measure(pieces, &measured_overflow);
        CHECK(measured_overflow == (extra == 1));   // the measuring pass already reports it: the call fails before it stages
        Images I(pieces);
        CHECK(I.st.out_overflow == (extra == 1) && I.st.n_out == Stage::kMaxOut);
        CHECK(I.total == (size_t)n * 256);          // a refused record still stages its piece
        if (!extra) {
            I.send();
            for (size_t i = 0; i < I.total; ++i) I.d[i] = 0x77;
            I.fetch();
            for (int i = 0; i < n; ++i) CHECK(hosts[i].all(0x77) && hosts[i].guards());
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    if (!strcmp(argv[1], "sizes")) sizes();
    else if (!strcmp(argv[1], "fillers")) fillers();
    else if (!strcmp(argv[1], "outputs")) outputs();
    else if (!strcmp(argv[1], "capacity")) capacity();
    else return 2;
    if (!g_failed) printf("ok\n");
    return g_failed ? 1 : 0;
}
