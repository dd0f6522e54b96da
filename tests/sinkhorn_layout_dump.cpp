// Prints the stream kernel's LDS layouts and the pass plans of the Sinkhorn grid call over a grid of shapes, one line of
// key=value fields per case, for tests/test_sinkhorn_layout.py.  Host C++ only: it includes nothing but the layout header.
#include <cstdio>
#include <initializer_list>

#include "../pilot_amd/csrc/sinkhorn_layout.hpp"

using namespace pilot;

static void print_layout(const char *pre, const StreamLayout &l) {
    printf(" %stable=%d %stail=%d %srings=%d %spark=%d %shb=%d %send=%d %sslot=%d %spanel=%d %slbytes=%zu", pre, l.table, pre, l.tail, pre, l.rings, pre, l.park, pre, l.hb, pre, l.end, pre, l.slot, pre, l.panel, pre, l.bytes);
}

static void print_pass(const char *pre, const PassPlan &v, int RT, bool sym) {
    const CfgShape c = shape_of(v.cfg);
    printf(" %srun=%d %scfg=%d %stv=%d %slive1=%d %strack=%d %squad=%d %ssolo64=%d %sbands=%d %sinherited=%zu %sbytes=%zu %sring=%d %swpc=%d %swgs=%d"
           " %ssolo_blocks=%d %slist=%d %slen=%d %shead=%d %sshards=%d %sw=%d",
           pre, v.run, pre, v.cfg, pre, v.tv, pre, v.live1, pre, v.track, pre, v.quad, pre, v.solo_f64, pre, v.bands, pre, v.inherited, pre, v.lds.bytes,
           pre, v.lds.ring, pre, v.lds.wgs_per_cu, pre, v.wgs, pre, v.solo_blocks, pre, (int)v.list, pre, v.len_slot, pre, v.head_slot, pre, v.shards_at, pre, c.w);
    // what the launch needs with no slot and with one slot per wave, and the kernel's layout at the planned ring
    printf(" %sfixed=%zu %sslots=%zu", pre, stream_layout(c, RT, sym, v.track, v.tv, v.bands, 0).bytes + v.inherited, pre,
           stream_layout(c, RT, sym, v.track, v.tv, v.bands, 1).bytes - stream_layout(c, RT, sym, v.track, v.tv, v.bands, 0).bytes);
    print_layout(pre, stream_layout(c, RT, sym, v.track, v.tv, v.bands, v.lds.ring));
}

int main() {
    const int cfgs[4] = {CFG_F32, CFG_F64, CFG_S32, CFG_H32};
    printf("C lds_bytes=%zu waves=%d wave=%d ring_max=%d handover=%d enotsup=%d cfg_f32=%d cfg_f64=%d cfg_s32=%d cfg_h32=%d no_solo=%d no_tail=%d no_track_all=%d\n",
           LDS_BYTES, WAVES_PER_WG, WAVE, RING_MAX, HANDOVER_BUF, PILOT_OT_ENOTSUP, CFG_F32, CFG_F64, CFG_S32, CFG_H32, DBG_NO_SOLO, DBG_NO_TAIL_ROWS,
           DBG_NO_TRACK_ALL);
    // every layout the kernels can be instantiated with, at the smallest, a middle and the largest ring
    for (int cfg : cfgs)
        for (int RT = 1; RT <= 8; ++RT)
            for (int sym = 0; sym < 2; ++sym)
                for (int track = 0; track < 2; ++track)
                    for (int bands = 1; bands <= 2; ++bands)
                        for (int tv = 0; tv <= 2; ++tv)
                            for (int ring : {1, 4, RING_MAX}) {
                                const CfgShape c = shape_of(cfg);
                                if (tv > 0 && (RT < 2 || (c.split && tv > 1))) continue;      // (TV needs two row-tiles; split: live1 only)
                                if (bands == 2 && !(cfg == CFG_S32 && track)) continue;
                                if (c.half && track) continue;
                                printf("L cfg=%d RT=%d sym=%d track=%d bands=%d tv=%d ring=%d w=%d", cfg, RT, sym, track, bands, tv, ring, c.w);
                                print_layout("", stream_layout(c, RT, sym != 0, track != 0, tv, bands, ring));
                                printf("\n");
                            }
    // (debug -1: no switch of PILOT_OT_DEBUG, PILOT_OT_NO_QUAD set)
    const int debugs[5] = {0, DBG_NO_SOLO, DBG_NO_TAIL_ROWS, DBG_NO_TRACK_ALL, -1};
    const double mcrs[4] = {10, 13, 25, 100};
    for (int cfg : cfgs)
        for (int RT = 1; RT <= 8; ++RT)
            for (int K : {16 * RT - 15, 16 * RT - 12, 16 * RT - 11, 16 * RT})
                for (int sym = 0; sym < 2; ++sym)
                    for (int mixed = 0; mixed <= (cfg == CFG_S32 ? 1 : 0); ++mixed)
                        for (int N : {1, 40, 600})
                            for (int n_rows : {N, 1})
                                for (double mcr : mcrs)
                                    for (int n_cu : {1, 256})
                                        for (int debug : debugs) {
                                            if (n_rows == 1 && N != 600) continue;     // (one row shard: at the largest grid only)
                                            const SinkhornSwitches sw = {debug < 0 ? 0 : debug, debug < 0 ? 1 : 0, 0};
                                            const GridPasses g = plan_grid(cfg, N, K, n_rows, sym != 0, mixed != 0, mcr, n_cu, sw);
                                            const CfgShape c = shape_of(cfg);
                                            const int tvf = c.split ? g.fast.live1 : g.fast.tv;
                                            printf("P cfg=%d K=%d RT=%d sym=%d mixed=%d N=%d n_rows=%d mcr=%g n_cu=%d debug=%d rc=%d mode=%d write_tail=%d ob=%d mw=%d"
                                                   " solo_rule=%d no_quad=%d mw_t=%d mw_d=%d",
                                                   cfg, K, RT, sym, mixed, N, n_rows, mcr, n_cu, sw.debug, g.rc, g.mode, g.write_tail, g.ob,
                                                   min_waves_per_simd(c, RT, sym != 0, false, tvf), (int)solo_in_stream(c, RT, sym != 0, false, tvf), sw.no_quad,
                                                   min_waves_per_simd(shape_of(g.track.cfg), RT, sym != 0, true, c.split ? g.track.live1 : g.track.tv),
                                                   min_waves_per_simd(shape_of(CFG_F64), RT, sym != 0, true, 0));
                                            print_pass("f_", g.fast, RT, sym != 0);
                                            print_pass("t_", g.track, RT, sym != 0);
                                            print_pass("d_", g.f64, RT, sym != 0);
                                            printf(" msg=%s\n", g.rc ? "set" : "none");
                                        }
    return 0;
}
