// Host build of orbhip_sim3opt_core.h: one thread replays what a device team does, so its outputs must equal those of
// tests/seqref/sim3opt.py bit for bit (tests/test_sim3opt_cpu.py builds this with g++ -ffp-contract=off and runs it).
//   sim3opt_host run <in> <out>      in:  int32 header {C, cur, rows, cap, np, pcap, match_form, n_levels, fix_scale, has select,
//                                         has Scw, observations}, float cam[4] = fx, fy, cx, cy, float th2, float
//                                         inv_level_sigma2[n_levels], then slot_point, n, obs_start, obs_kf, obs_idx, flags,
//                                         world, Tcw, kps, kf_index, [select], matched12, sim3, S12, [Scw], report as the C ABI
//                                         lays them out
//                                    out: matched12, S12, [Scw], report, then the estimate and the last tried estimate of the
//                                         last candidate that ran as 2 x 8 doubles (quaternion x y z w, t, s)
//   sim3opt_host classify <in> <out> in:  as for run, followed by double tried[8] and uint8 e_out[cap]: the check after a
//                                         round (s3o_classify) of candidate 0 with that state
//                                    out: uint8 e_out[cap], int32 matched12[cap], int32 removed, int32 pairs
//   sim3opt_host exp <in> <out>      in: doubles; out: det_exp64 of each
//   run and classify take an optional trailing argument: the byte (0 .. 255, default 0) that the team's record S3oWs (its two
//   emitted estimates start at zero all the same) and the pair lists e_slot, e_i2, e_p2, e_out hold before the run
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbhip_sim3opt_core.h"

using namespace orbhip;

static std::vector<unsigned char> slurp(const char *path)
{
    std::vector<unsigned char> v;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

struct Cursor {
    std::vector<unsigned char> &v;
    size_t off;
    // a copy: the arrays follow each other without padding, so they are not aligned inside the file
    template <class T> std::vector<T> take(size_t count)
    {
        const size_t bytes = count * sizeof(T);
        if (off + bytes > v.size()) { fprintf(stderr, "input too short\n"); exit(2); }
        std::vector<T> r(count);
        if (bytes) memcpy(r.data(), v.data() + off, bytes);
        off += bytes;
        return r;
    }
};

template <class T> static void emit(FILE *f, const T *p, size_t count)
{
    if (fwrite(p, sizeof(T), count, f) != count) { perror("write"); exit(2); }
}

int main(int argc, char **argv)
{
    if (argc != 4 && argc != 5) { fprintf(stderr, "usage: sim3opt_host run|classify|exp <in> <out> [fill]\n"); return 2; }
    const uint8_t fill = argc == 5 ? (uint8_t)strtol(argv[4], nullptr, 0) : 0;
    std::vector<unsigned char> in = slurp(argv[2]);
    FILE *out = fopen(argv[3], "wb");
    if (!out) { perror(argv[3]); return 2; }
    if (argv[1][0] == 'e') {
        const size_t cnt = in.size() / sizeof(double);
        std::vector<double> x(cnt), r(cnt);
        if (cnt) memcpy(x.data(), in.data(), cnt * sizeof(double));
        for (size_t i = 0; i < cnt; ++i) r[i] = det_exp64(x[i]);
        emit(out, r.data(), r.size());
        fclose(out);
        return 0;
    }
    Cursor c{in, 0};
    const std::vector<int32_t> h = c.take<int32_t>(12);
    const int C = h[0], cur = h[1], rows = h[2], cap = h[3], np = h[4], pcap = h[5], match_form = h[6], n_levels = h[7], fix_scale = h[8];
    const size_t total = (size_t)h[11];
    if (C < 0 || rows < 1 || cur < 0 || cur >= rows || cap < 1 || cap > kS3oCapMax || np < 0 || np > pcap || n_levels < 1 ||
        n_levels > ORBHIP_MAX_LEVELS || h[11] < 0)
        return 2;
    const std::vector<float> cam = c.take<float>(4), th2 = c.take<float>(1), inv = c.take<float>(n_levels);
    const size_t RC = (size_t)rows * cap, Cn = (size_t)C, CC = Cn * cap;
    const std::vector<int32_t> slot_point = c.take<int32_t>(RC), n = c.take<int32_t>(rows), obs_start = c.take<int32_t>((size_t)np + 1);
    const std::vector<int32_t> obs_kf = c.take<int32_t>(total), obs_idx = c.take<int32_t>(total);
    const std::vector<uint8_t> flags = c.take<uint8_t>(pcap);
    const std::vector<float> world = c.take<float>((size_t)pcap * 3), Tcw = c.take<float>((size_t)rows * 12);
    const std::vector<orbhip_keypoint> kps = c.take<orbhip_keypoint>(RC);
    const std::vector<int32_t> kf_index = c.take<int32_t>(Cn);
    const std::vector<uint8_t> select = c.take<uint8_t>(h[9] ? Cn : 0);
    std::vector<int32_t> matched = c.take<int32_t>(CC);
    const std::vector<float> sim3 = c.take<float>(Cn * 16);
    std::vector<double> S12 = c.take<double>(Cn * 8);
    std::vector<float> Scw = c.take<float>(h[10] ? Cn * 12 : 0);
    std::vector<int32_t> report = c.take<int32_t>(Cn * 8);
    const bool classify = argv[1][0] == 'c';
    const std::vector<double> state = c.take<double>(classify ? 8 : 0);
    const std::vector<uint8_t> flags_in = c.take<uint8_t>(classify ? (size_t)cap : 0);
    if (obs_start[0] != 0 || (size_t)obs_start[np] != total) return 2;
    S3oTables T;
    T.slot_point = slot_point.data(); T.n = n.data(); T.obs_start = obs_start.data(); T.obs_kf = obs_kf.data();
    T.obs_idx = obs_idx.data(); T.flags = flags.data();
    T.rows = rows; T.cap = cap; T.np = np; T.cur = cur; T.match_form = match_form;
    std::vector<uint16_t> e_slot(cap), e_i2(cap);
    std::vector<int> e_p2(cap);
    std::vector<uint8_t> e_out(cap, fill);
    memset(e_slot.data(), fill, e_slot.size() * sizeof(uint16_t));
    memset(e_i2.data(), fill, e_i2.size() * sizeof(uint16_t));
    memset(e_p2.data(), fill, e_p2.size() * sizeof(int));
    static S3oWs W;
    memset(&W, fill, sizeof(W));
    for (int k = 0; k < 8; ++k) W.est[k] = W.tried[k] = 0.0;
    for (int cd = 0; cd < C; ++cd) {
        if (h[9] && !select[cd]) { report[(size_t)cd * 8] = ORBHIP_SIM3OPT_SKIPPED; continue; }
        const int kf = kf_index[cd];
        if (kf < 0 || kf >= rows) return 2;
        S3oCand F;
        F.kps_cur = kps.data() + (size_t)cur * cap;
        F.kps_kf = kps.data() + (size_t)kf * cap;
        F.sp_cur = slot_point.data() + (size_t)cur * cap;
        F.world = world.data();
        F.T1 = Tcw.data() + (size_t)cur * 12;
        F.T2 = Tcw.data() + (size_t)kf * 12;
        F.inv_sigma2 = inv.data();
        F.sim3 = sim3.data() + (size_t)cd * 16;
        F.matched = matched.data() + (size_t)cd * cap;
        F.S12 = S12.data() + (size_t)cd * 8;
        F.Scw = h[10] ? Scw.data() + (size_t)cd * 12 : nullptr;
        F.report = report.data() + (size_t)cd * 8;
        F.e_slot = e_slot.data(); F.e_i2 = e_i2.data(); F.e_p2 = e_p2.data(); F.e_out = e_out.data();
        F.n_levels = n_levels; F.fix_scale = fix_scale;
        F.cam.fx = (double)cam[0]; F.cam.fy = (double)cam[1]; F.cam.cx = (double)cam[2]; F.cam.cy = (double)cam[3];
        F.delta = (double)std::sqrt(th2[0]);
        F.dsqr = F.delta * F.delta;
        F.th2 = (double)th2[0];
        s3o_host_compact(W, T, kf, F);
        S3oHostTeam tm;
        if (classify) {
            for (int k = 0; k < 8; ++k) W.tried[k] = state[k];
            s3o_inverse(W.tried, W.tinv);
            for (int j = 0; j < W.ne; ++j) e_out[j] = flags_in[j];
            const int32_t counts[2] = {s3o_classify(tm, W, F, W.ne), W.ne};
            emit(out, e_out.data(), (size_t)cap);
            emit(out, F.matched, (size_t)cap);
            emit(out, counts, 2);
            fclose(out);
            return 0;
        }
        s3o_run(tm, W, F);
    }
    emit(out, matched.data(), CC);
    emit(out, S12.data(), Cn * 8);
    if (h[10]) emit(out, Scw.data(), Cn * 12);
    emit(out, report.data(), report.size());
    emit(out, W.est, 8);
    emit(out, W.tried, 8);
    fclose(out);
    return 0;
}
