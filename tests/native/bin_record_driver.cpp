// Drives awsm-renderer_amd/csrc/bin_record.hpp on the CPU (tests/test_bin_record_cpu.py): reads commands from stdin, prints results.
//   p <ok> <big> <tx0> <ty0> <wm1> <hm1> <mask>   pack, then unpack what was packed: "<w0> <w1>  <ok> <big> <tx0> <ty0> <wm1> <hm1> <mask>"
//   u <w0> <w1>                                   unpack: "<ok> <big> <tx0> <ty0> <wm1> <hm1> <mask>"
//   f <tiles_x> <tiles_y>                         bin_rec_fits: 0 / 1
//   k                                             the constants: "<tiles> <extent bits> <tile bits> <max cols> <max rows>"
#include <cstdio>
#include <cstring>
#include "../../awsm-renderer_amd/csrc/bin_record.hpp"
static void show(const awsm::BinRec& r) { printf("%u %u %u %u %u %u %u\n", r.ok ? 1u : 0u, r.big ? 1u : 0u, r.tx0, r.ty0, r.wm1, r.hm1, r.mask); }
int main() {
    char op[8];
    while (scanf("%7s", op) == 1) {
        if (!strcmp(op, "p")) {
            unsigned ok, big; awsm::BinRec r;
            if (scanf("%u %u %u %u %u %u %u", &ok, &big, &r.tx0, &r.ty0, &r.wm1, &r.hm1, &r.mask) != 7) return 2;
            r.ok = ok != 0; r.big = big != 0;
            const awsm::BinRecWords w = awsm::bin_rec_pack(r);
            printf("%u %u  ", w.w0, w.w1);
            show(awsm::bin_rec_unpack(w));
        } else if (!strcmp(op, "u")) {
            awsm::BinRecWords w;
            if (scanf("%u %u", &w.w0, &w.w1) != 2) return 2;
            show(awsm::bin_rec_unpack(w));
        } else if (!strcmp(op, "f")) {
            unsigned x, y; if (scanf("%u %u", &x, &y) != 2) return 2;
            printf("%d\n", awsm::bin_rec_fits(x, y) ? 1 : 0);
        } else if (!strcmp(op, "k")) {
            printf("%u %u %u %u %u\n", awsm::kBinRecTiles, awsm::kBinRecExtentBits, awsm::kBinRecTileBits, awsm::kBinRecMaxTileCols, awsm::kBinRecMaxTileRows);
        } else return 2;
    }
    return 0;
}
