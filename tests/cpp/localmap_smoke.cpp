// The local-map call of the C++ mirror (include/orbhip/ORBextractor.hpp: UpdateLocalMap) the way Tracking::UpdateLocalMap
// and SearchLocalPoints use it (src/Tracking.cc:1146-1180, :1205-1339).  Reads "frames rows cap np pcap nchild nobs" as
// int32, then slotPoint[rows][cap], n[rows], kfBad[rows], covis[rows][10], childStart[rows+1], child[nchild], parent[rows],
// obsStart[np+1], obsKf[nobs], flags[pcap], world[pcap][3], normal[pcap][3], maxDist[pcap], minDist[pcap],
// pointDesc[pcap][32], framePoint[frames][cap], frameN[frames], localKf[frames][rows], nLocalKf[frames]; writes the in/out
// and output arrays of orbhip_local_map_io in the record's order, the outputs pre-filled with 0x5a bytes.
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
    if (argc < 3) { std::fprintf(stderr, "usage: localmap_smoke in.bin out.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[7];
    if (std::fread(hdr, 4, 7, f) != 7) return 3;
    const size_t frames = (size_t)hdr[0], rows = (size_t)hdr[1], cap = (size_t)hdr[2], np = (size_t)hdr[3], pcap = (size_t)hdr[4];
    const size_t nchild = (size_t)hdr[5], nobs = (size_t)hdr[6];
    std::vector<int32_t> slotPoint, n, covis, childStart, child, parent, obsStart, obsKf, framePoint, frameN, localKf, nLocalKf;
    std::vector<uint8_t> kfBad, flags, pointDesc;
    std::vector<float> world, normal, maxDist, minDist;
    if (!rd(f, slotPoint, rows * cap) || !rd(f, n, rows) || !rd(f, kfBad, rows) || !rd(f, covis, rows * 10) ||
        !rd(f, childStart, rows + 1) || !rd(f, child, nchild) || !rd(f, parent, rows) || !rd(f, obsStart, np + 1) ||
        !rd(f, obsKf, nobs) || !rd(f, flags, pcap) || !rd(f, world, 3 * pcap) || !rd(f, normal, 3 * pcap) || !rd(f, maxDist, pcap) ||
        !rd(f, minDist, pcap) || !rd(f, pointDesc, 32 * pcap) || !rd(f, framePoint, frames * cap) || !rd(f, frameN, frames) ||
        !rd(f, localKf, frames * rows) || !rd(f, nLocalKf, frames))
        return 3;
    std::fclose(f);
    child.resize(nchild + 1);   // a required pointer even when no row has a child
    obsKf.resize(nobs + 1);
    const int32_t fillI = 0x5a5a5a5a;
    float fillF;
    std::memcpy(&fillF, &fillI, 4);
    std::vector<int32_t> votes(frames * rows, fillI), localPoint(frames * pcap, fillI), npL(frames, fillI), report(frames * 8, fillI);
    std::vector<float> worldL(frames * pcap * 3, fillF), normalL(frames * pcap * 3, fillF), maxDistL(frames * pcap, fillF),
        minDistL(frames * pcap, fillF);
    std::vector<uint8_t> descL(frames * pcap * 32, 0x5a), flagsL(frames * pcap, 0x5a), taken(frames * cap, 0x5a);
    orbhip_local_map_tables t;
    t.slot_point = slotPoint.data(); t.n = n.data(); t.kf_bad = kfBad.data(); t.covis = covis.data();
    t.child_start = childStart.data(); t.child = child.data(); t.parent = parent.data(); t.obs_start = obsStart.data();
    t.obs_kf = obsKf.data(); t.flags = flags.data(); t.world = world.data(); t.normal = normal.data(); t.max_dist = maxDist.data();
    t.min_dist = minDist.data(); t.point_desc = pointDesc.data();
    orbhip_local_map_io io;
    io.frame_point = framePoint.data(); io.frame_n = frameN.data(); io.local_kf = localKf.data(); io.n_local_kf = nLocalKf.data();
    io.votes = votes.data(); io.local_point = localPoint.data(); io.world_l = worldL.data(); io.normal_l = normalL.data();
    io.max_dist_l = maxDistL.data(); io.min_dist_l = minDistL.data(); io.desc_l = descL.data(); io.flags_l = flagsL.data();
    io.np_l = npL.data(); io.taken = taken.data(); io.report = report.data();
    try {
        orbhip::ORBmatcher matcher(0.8f, true);
        matcher.UpdateLocalMap((int)frames, (int)rows, (int)cap, (int)np, (int)pcap, t, io);
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 3;
        wr(o, framePoint); wr(o, localKf); wr(o, nLocalKf); wr(o, votes); wr(o, localPoint); wr(o, worldL); wr(o, normalL);
        wr(o, maxDistL); wr(o, minDistL); wr(o, descL); wr(o, flagsL); wr(o, npL); wr(o, taken); wr(o, report);
        std::fclose(o);
        for (size_t fr = 0; fr < frames; ++fr)
            std::printf("frame %zu status %d local key frames %d local points %d\n", fr, report[fr * 8], report[fr * 8 + 2],
                        report[fr * 8 + 6]);
        // a row outside the bank, a count over the capacity and a null table: refused, nothing changed
        const std::vector<int32_t> before = localPoint;
        if (nobs) {
            const int32_t keep = obsKf[0];
            obsKf[0] = (int32_t)rows;
            try { matcher.UpdateLocalMap((int)frames, (int)rows, (int)cap, (int)np, (int)pcap, t, io); return 6; }
            catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
            obsKf[0] = keep;
        }
        try { matcher.UpdateLocalMap((int)frames, (int)rows, 4097, (int)np, (int)pcap, t, io); return 6; }
        catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_CAPACITY) return 6; }
        orbhip_local_map_tables t2 = t;
        t2.parent = nullptr;
        try { matcher.UpdateLocalMap((int)frames, (int)rows, (int)cap, (int)np, (int)pcap, t2, io); return 6; }
        catch (const orbhip::Error &e) { if (e.code != ORBHIP_E_ARG) return 6; }
        if (localPoint != before) return 7;
    } catch (const orbhip::Error &e) {
        std::fprintf(stderr, "orbhip error %d: %s\n", e.code, e.what());
        return 5;
    }
    return 0;
}
