// The covisibility calls of the C++ mirror (include/orbhip/ORBextractor.hpp: UpdateConnections, CovisibleTargets) the way
// LocalMapping::ProcessNewKeyFrame and SearchInNeighbors use them (src/KeyFrame.cc:289-379, src/LocalMapping.cc:457-479).
// Reads "rows cap np pcap nobs U id0 Q nn nn2" as int32, then slotPoint[rows][cap], n[rows], obsStart[np+1], obsKf[nobs],
// flags[pcap], connW[rows][rows], ordKf[rows][rows], ordW[rows][rows], nOrd[rows], covis[rows][10], firstConn[rows],
// parent[rows], updateRows[U], kfBad[rows], cur[Q]; writes the seven state arrays in the record's order, report[U][8],
// targets[Q][nn * (1 + nn2)] and counts[Q], the outputs pre-filled with 0x5a bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip/ORBextractor.hpp"

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T> static void wr(FILE *f, const std::vector<T> &v) { std::fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: covisibility_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[10];
    if (std::fread(hdr, 4, 10, f) != 10) return 3;
    const size_t rows = (size_t)hdr[0], cap = (size_t)hdr[1], np = (size_t)hdr[2], pcap = (size_t)hdr[3], nobs = (size_t)hdr[4];
    const size_t U = (size_t)hdr[5], Q = (size_t)hdr[7];
    const int id0 = hdr[6], nn = hdr[8], nn2 = hdr[9];
    std::vector<int32_t> slotPoint, n, obsStart, obsKf, connW, ordKf, ordW, nOrd, covis, parent, updateRows, cur;
    std::vector<uint8_t> flags, firstConn, kfBad;
    if (!rd(f, slotPoint, rows * cap) || !rd(f, n, rows) || !rd(f, obsStart, np + 1) || !rd(f, obsKf, nobs) || !rd(f, flags, pcap) ||
        !rd(f, connW, rows * rows) || !rd(f, ordKf, rows * rows) || !rd(f, ordW, rows * rows) || !rd(f, nOrd, rows) ||
        !rd(f, covis, rows * 10) || !rd(f, firstConn, rows) || !rd(f, parent, rows) || !rd(f, updateRows, U) || !rd(f, kfBad, rows) ||
        !rd(f, cur, Q))
        return 3;
    std::fclose(f);
    obsKf.resize(nobs + 1);   // a required pointer even when nobody observes anything
    const int32_t fillI = 0x5a5a5a5a;
    const size_t width = (size_t)nn * (1 + (size_t)nn2);
    std::vector<int32_t> report(U * 8, fillI), targets(Q * width, fillI), counts(Q, fillI);
    orbhip_covis_tables t;
    t.slot_point = slotPoint.data(); t.n = n.data(); t.obs_start = obsStart.data(); t.obs_kf = obsKf.data(); t.flags = flags.data();
    orbhip_covis_state s;
    s.conn_w = connW.data(); s.ord_kf = ordKf.data(); s.ord_w = ordW.data(); s.n_ord = nOrd.data(); s.covis = covis.data();
    s.first_conn = firstConn.data(); s.parent = parent.data();
    try {
        orbhip::ORBmatcher matcher(0.6f, true);
        matcher.UpdateConnections((int)rows, (int)cap, (int)np, (int)pcap, t, s, id0, (int)U, updateRows.data(), report.data());
        matcher.CovisibleTargets((int)rows, ordKf.data(), nOrd.data(), kfBad.data(), (int)Q, cur.data(), nn, nn2, targets.data(),
                                 counts.data());
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 3;
        wr(o, connW); wr(o, ordKf); wr(o, ordW); wr(o, nOrd); wr(o, covis); wr(o, firstConn); wr(o, parent); wr(o, report);
        wr(o, targets); wr(o, counts);
        std::fclose(o);
        for (size_t u = 0; u < U; ++u)
            std::printf("entry %zu row %d status %d ordered %d parent %d\n", u, updateRows[u], report[u * 8], report[u * 8 + 2],
                        report[u * 8 + 5]);
        // a row outside the bank, a bank over the limit and a null table: refused, nothing changed
        const std::vector<int32_t> before = connW;
        if (U) {
            const int32_t keep = updateRows[0];
            updateRows[0] = (int32_t)rows;
            try { matcher.UpdateConnections((int)rows, (int)cap, (int)np, (int)pcap, t, s, id0, (int)U, updateRows.data(), report.data()); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
            updateRows[0] = keep;
        }
        try { matcher.UpdateConnections(4097, (int)cap, (int)np, (int)pcap, t, s, -1, (int)U, updateRows.data(), report.data()); return 6; }
        catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_CAPACITY) return 6; }
        orbhip_covis_state s2 = s;
        s2.parent = nullptr;
        try { matcher.UpdateConnections((int)rows, (int)cap, (int)np, (int)pcap, t, s2, id0, (int)U, updateRows.data(), report.data()); return 6; }
        catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        if (connW != before) return 7;
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
