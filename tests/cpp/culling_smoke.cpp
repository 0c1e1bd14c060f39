// The culling calls of the C++ mirror (include/orbhip/ORBextractor.hpp: CullMapPoints, CullKeyFrames) the way
// LocalMapping::Run uses them (src/LocalMapping.cc:170-205, :632-696): the map points first, the table out swapped in, then
// the key frames.  Reads "rows cap np pcap obsCap U id0 R mono thObs curKfId stereo" as int32 and thDepth as float, then
// octave[rows][cap], uRight[rows][cap] (stereo only), depth[rows][cap], n[rows], obsStart[np+1], obsKf[obsCap], obsIdx[obsCap],
// refObs[np], notErase[rows], slotPoint[rows][cap], flags[pcap], kfBad[rows], toBeErased[rows], childStart[rows+1], child[rows],
// connW / ordKf / ordW [rows][rows], nOrd[rows], covis[rows][10], firstConn[rows], parent[rows], cand[U], recent[R],
// found / visible / firstKfId [pcap]; writes status[R], nRecentOut, recentOut[R], the table after the first call, then
// slotPoint, flags, kfBad, toBeErased, childStart, child, the table after the second call, connW, ordKf, ordW, nOrd, covis,
// parent and report[U][8]; outputs are pre-filled with 0x5a bytes.
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
    if (argc < 3) { std::fprintf(stderr, "usage: culling_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[12];
    float thDepth;
    if (std::fread(hdr, 4, 12, f) != 12 || std::fread(&thDepth, 4, 1, f) != 1) return 3;
    const size_t rows = (size_t)hdr[0], cap = (size_t)hdr[1], np = (size_t)hdr[2], pcap = (size_t)hdr[3], obsCap = (size_t)hdr[4];
    const size_t U = (size_t)hdr[5], R = (size_t)hdr[7];
    const int id0 = hdr[6], mono = hdr[8], thObs = hdr[9], curKfId = hdr[10], stereo = hdr[11];
    std::vector<int32_t> octave, n, obsStart, obsKf, obsIdx, refObs, slotPoint, childStart, child, connW, ordKf, ordW, nOrd, covis, parent,
        cand, recent, found, visible, firstKfId;
    std::vector<float> uRight, depth;
    std::vector<uint8_t> notErase, flags, kfBad, toBeErased, firstConn;
    if (!rd(f, octave, rows * cap) || !rd(f, uRight, stereo ? rows * cap : 0) || !rd(f, depth, rows * cap) || !rd(f, n, rows) ||
        !rd(f, obsStart, np + 1) || !rd(f, obsKf, obsCap) || !rd(f, obsIdx, obsCap) || !rd(f, refObs, np) || !rd(f, notErase, rows) ||
        !rd(f, slotPoint, rows * cap) || !rd(f, flags, pcap) || !rd(f, kfBad, rows) || !rd(f, toBeErased, rows) ||
        !rd(f, childStart, rows + 1) || !rd(f, child, rows) || !rd(f, connW, rows * rows) || !rd(f, ordKf, rows * rows) ||
        !rd(f, ordW, rows * rows) || !rd(f, nOrd, rows) || !rd(f, covis, rows * 10) || !rd(f, firstConn, rows) || !rd(f, parent, rows) ||
        !rd(f, cand, U) || !rd(f, recent, R) || !rd(f, found, pcap) || !rd(f, visible, pcap) || !rd(f, firstKfId, pcap))
        return 3;
    std::fclose(f);
    std::vector<orbhip_keypoint> kps(rows * cap);
    std::memset(kps.data(), 0, kps.size() * sizeof(orbhip_keypoint));
    for (size_t i = 0; i < rows * cap; ++i) kps[i].octave = octave[i];
    const int32_t fillI = 0x5a5a5a5a;
    std::vector<int32_t> start1(np + 1, fillI), kf1(obsCap, fillI), idx1(obsCap, fillI), ref1(np, fillI);
    std::vector<int32_t> start2(np + 1, fillI), kf2(obsCap, fillI), idx2(obsCap, fillI), ref2(np, fillI);
    std::vector<int32_t> recentOut(R, fillI), nRecentOut(1, fillI), report(U * 8, fillI);
    std::vector<uint8_t> status(R, 0x5a);
    orbhip_cull_tables t;
    std::memset(&t, 0, sizeof(t));
    t.kps = kps.data(); t.u_right = stereo ? uRight.data() : nullptr; t.depth = depth.data(); t.n = n.data();
    t.obs_start = obsStart.data(); t.obs_kf = obsKf.data(); t.obs_idx = obsIdx.data(); t.ref_obs = refObs.data();
    t.not_erase = notErase.data();
    orbhip_cull_io io;
    io.slot_point = slotPoint.data(); io.flags = flags.data(); io.kf_bad = kfBad.data(); io.to_be_erased = toBeErased.data();
    io.child_start = childStart.data(); io.child = child.data();
    io.obs_start_out = start1.data(); io.obs_kf_out = kf1.data(); io.obs_idx_out = idx1.data(); io.ref_obs_out = ref1.data();
    orbhip_covis_state s;
    s.conn_w = connW.data(); s.ord_kf = ordKf.data(); s.ord_w = ordW.data(); s.n_ord = nOrd.data(); s.covis = covis.data();
    s.first_conn = firstConn.data(); s.parent = parent.data();
    try {
        orbhip::ORBmatcher matcher(0.6f, true);
        matcher.CullMapPoints((int)rows, (int)cap, (int)np, (int)pcap, (int)obsCap, t, io, (int)R, recent.data(), found.data(),
                              visible.data(), firstKfId.data(), curKfId, thObs, recentOut.data(), nRecentOut.data(), status.data());
        // the table out becomes the table in
        orbhip_cull_tables t2 = t;
        t2.obs_start = start1.data(); t2.obs_kf = kf1.data(); t2.obs_idx = idx1.data(); t2.ref_obs = ref1.data();
        orbhip_cull_io io2 = io;
        io2.obs_start_out = start2.data(); io2.obs_kf_out = kf2.data(); io2.obs_idx_out = idx2.data(); io2.ref_obs_out = ref2.data();
        matcher.CullKeyFrames((int)rows, (int)cap, (int)np, (int)pcap, (int)obsCap, t2, io2, s, id0, (int)U, cand.data(), mono != 0,
                              thDepth, report.data());
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 3;
        wr(o, status); wr(o, nRecentOut); wr(o, recentOut); wr(o, start1); wr(o, kf1); wr(o, idx1); wr(o, ref1);
        wr(o, slotPoint); wr(o, flags); wr(o, kfBad); wr(o, toBeErased); wr(o, childStart); wr(o, child);
        wr(o, start2); wr(o, kf2); wr(o, idx2); wr(o, ref2);
        wr(o, connW); wr(o, ordKf); wr(o, ordW); wr(o, nOrd); wr(o, covis); wr(o, parent); wr(o, report);
        std::fclose(o);
        std::printf("recent %zu kept %d\n", R, nRecentOut[0]);
        for (size_t u = 0; u < U; ++u)
            std::printf("candidate %zu row %d status %d points %d redundant %d\n", u, cand[u], report[u * 8], report[u * 8 + 1],
                        report[u * 8 + 2]);
        // a candidate outside the bank, a bank over the limit and an aliased table: refused, nothing changed
        const std::vector<int32_t> before = slotPoint;
        if (U) {
            const int32_t keep = cand[0];
            cand[0] = (int32_t)rows;
            try { matcher.CullKeyFrames((int)rows, (int)cap, (int)np, (int)pcap, (int)obsCap, t2, io2, s, id0, (int)U, cand.data(), mono != 0, thDepth, report.data()); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
            cand[0] = keep;
        }
        try { matcher.CullKeyFrames(4097, (int)cap, (int)np, (int)pcap, (int)obsCap, t2, io2, s, -1, (int)U, cand.data(), mono != 0, thDepth, report.data()); return 6; }
        catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_CAPACITY) return 6; }
        orbhip_cull_io io3 = io2;
        io3.obs_kf_out = kf1.data();
        try { matcher.CullMapPoints((int)rows, (int)cap, (int)np, (int)pcap, (int)obsCap, t2, io3, (int)R, recent.data(), found.data(), visible.data(), firstKfId.data(), curKfId, thObs, recentOut.data(), nRecentOut.data(), status.data()); return 6; }
        catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        if (slotPoint != before) return 7;
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
