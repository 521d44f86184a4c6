// flacdec_host_main.cpp -- the device FLAC decoder's core (csrc/amx_flacdec_core.hpp) on
// the CPU: test infrastructure for tests/test_flac_decode_core.py, built with
// g++ -fsanitize=address,undefined together with csrc/amx_flac.cpp (for amx_flac_scan, the
// same host scan the device path uses, and amx_flac_decode, the yardstick).
//
// Every candidate is decoded with the shared core into a heap block of exactly its size (so
// the sanitizer sees any write past a slot) from a heap copy of exactly the file's size (so
// it sees any read past the input); the frames are chained as k_flacd_chain chains them and
// emitted as k_flacd_emit emits them.
//
//   flacdec_host_main decode IN.flac OUT.i32 OUT.blocks
//       exit 0: decoded; 2: corrupt (the host path's AMX_EINVAL); 3: not supported by this path
//   flacdec_host_main fuzz IN.flac SEED N_FLIPS N_CUTS
//       N_FLIPS single-byte corruptions and N_CUTS truncations at seeded places, each decoded
//       by the core and by amx_flac_decode.  Where the host decoder accepts the stream the
//       core must give the same samples and blocks, unless it refused the frame the chain
//       stopped at for a width rule (amx.h: stricter than the host on invalid streams).
//       exit 0 and a line of counts, or 1 and the first disagreement.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/amx.h"
#include "../audio-mastering-engine_amd/csrc/amx_flacdec_core.hpp"

namespace {

struct HostStore {
    int32_t *slot = nullptr;   // C planes of exactly `block` samples
    int block = 0, wasted = 0;
    int32_t *plane = nullptr;
    int32_t cf[32];
    bool width = false;
    void begin(int channel, int w) {
        plane = slot + (size_t)channel * block;
        wasted = w;
    }
    void put(int i, int32_t v) { plane[i] = v; }
    int32_t get(int i) const { return plane[i]; }
    void finish(int n) {
        for (int i = 0; i < n; i++) plane[i] = (int32_t)((uint32_t)plane[i] << wasted);
    }
    void coef_set(int k, int32_t c) { cf[k] = c; }
    int32_t coef(int k) const { return cf[k]; }
    void out_of_width() { width = true; }
};

struct Result {
    int status = AMX_EINVAL;
    bool width_stop = false;   // the chain stopped at a frame refused for a width rule
    std::vector<int32_t> pcm, blocks;
};

// the device path, step by step, on d[0 .. size) (an exact-size heap block)
Result decode(const uint8_t *d, int64_t size) {
    Result R;
    amx_flac_scan_t sc;
    int rc = amx_flac_scan(d, size, nullptr, 0, &sc);
    if (rc != AMX_ERANGE) {
        R.status = rc == AMX_OK ? AMX_EINVAL : rc;
        return R;
    }
    std::vector<amx_flac_cand_t> cand((size_t)sc.n_cand);
    rc = amx_flac_scan(d, size, cand.data(), sc.n_cand, &sc);
    if (rc != AMX_OK) {
        R.status = rc;
        return R;
    }
    const int64_t nc = sc.n_cand;
    const int C = sc.channels;
    uint16_t tab[256];
    for (int i = 0; i < 256; i++) tab[i] = flacd::crc16_entry(i);
    // k_flacd_frames
    std::vector<int32_t *> slots((size_t)nc, nullptr);
    std::vector<int32_t> flag((size_t)nc, 0), nxt((size_t)nc, -1);
    std::vector<char> width((size_t)nc, 0);
    for (int64_t k = 0; k < nc; k++) {
        const amx_flac_cand_t &c = cand[(size_t)k];
        if (c.bps > 24) {
            flag[(size_t)k] = 2;
            continue;
        }
        slots[(size_t)k] = (int32_t *)std::malloc((size_t)c.block * C * sizeof(int32_t));
        HostStore st;
        st.slot = slots[(size_t)k];
        st.block = c.block;
        int64_t e = 0;
        if (flacd::decode_frame(d, size, c.offset, c.data_byte, c.limit, c.block, c.bps, c.assign, C, st, tab, &e)) {
            flag[(size_t)k] = 1;
            if (e < size) {
                int64_t lo = k + 1, hi = nc;
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (cand[(size_t)mid].offset < e) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < nc && cand[(size_t)lo].offset == e) nxt[(size_t)k] = (int32_t)lo;
            }
        }
        width[(size_t)k] = st.width;
    }
    // k_flacd_chain
    std::vector<int32_t> chain((size_t)nc);
    std::vector<int64_t> first((size_t)nc);
    R.blocks.resize((size_t)nc);
    int64_t samples = 0, stop = -1;
    const int64_t n = flacd::walk_chain(
        nc, [&](int64_t k) { return flag[(size_t)k]; }, [&](int64_t k) { return (int64_t)nxt[(size_t)k]; },
        [&](int64_t k) { return cand[(size_t)k].block; }, nc, chain.data(), first.data(), R.blocks.data(), &samples,
        &stop);
    R.blocks.resize((size_t)n);
    int status = AMX_OK;
    if (cand[0].offset != sc.first_frame) status = AMX_EINVAL;
    else if (stop >= 0 && flag[(size_t)stop] == 2) status = AMX_EUNSUPPORTED;
    else {
        if (samples > sc.total_frames) samples = sc.total_frames;
        if (samples < sc.total_frames) status = AMX_EINVAL;
    }
    R.status = status;
    R.width_stop = stop >= 0 && width[(size_t)stop];
    // k_flacd_emit
    if (status == AMX_OK) {
        R.pcm.resize((size_t)(samples * C));
        for (int64_t q = 0; q < n; q++) {
            const amx_flac_cand_t &c = cand[(size_t)chain[(size_t)q]];
            const int32_t *p = slots[(size_t)chain[(size_t)q]];
            const int64_t f0 = first[(size_t)q];
            const int take = (int)std::max<int64_t>(0, std::min<int64_t>(c.block, samples - f0));
            const int sh = 32 - c.bps;
            for (int i = 0; i < take; i++) {
                int32_t v[8];
                for (int ch = 0; ch < C; ch++) v[ch] = p[(size_t)ch * c.block + i];
                if (C == 2) flacd::undo_stereo(c.assign, p[i], p[(size_t)c.block + i], v[0], v[1]);
                for (int ch = 0; ch < C; ch++) R.pcm[(size_t)((f0 + i) * C + ch)] = (int32_t)((uint32_t)v[ch] << sh);
            }
        }
    }
    for (int32_t *s : slots) std::free(s);
    return R;
}

bool read_file(const char *path, std::vector<uint8_t> &v) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n);
    const bool ok = n == 0 || std::fread(v.data(), 1, (size_t)n, f) == (size_t)n;
    std::fclose(f);
    return ok;
}

bool write_file(const char *path, const void *p, size_t bytes) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

// on an exact-size heap copy, so a read one byte past the stream is a sanitizer report
Result decode_copy(const uint8_t *src, size_t n) {
    uint8_t *d = (uint8_t *)std::malloc(n ? n : 1);
    std::memcpy(d, src, n);
    Result R = decode(d, (int64_t)n);
    std::free(d);
    return R;
}

uint64_t rng_state;
uint64_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// 0: consistent; 1: the host accepts and the core disagrees without a width reason
int compare(const std::vector<uint8_t> &b, int counts[5]) {
    Result R = decode_copy(b.data(), b.size());
    int64_t frames = 0, nb = 0;
    int hrc = amx_flac_decode(b.data(), (int64_t)b.size(), nullptr, 0, &frames, 2, nullptr, 0, &nb);
    std::vector<int32_t> pcm, blocks;
    amx_flac_info_t info;
    if (hrc == AMX_OK && amx_flac_info(b.data(), (int64_t)b.size(), &info) == AMX_OK && frames > 0) {
        pcm.resize((size_t)(frames * info.channels));
        blocks.resize((size_t)nb);
        int64_t got = 0;
        hrc = amx_flac_decode(b.data(), (int64_t)b.size(), pcm.data(), frames, &got, 2, blocks.data(), nb, &nb);
        if (hrc == AMX_OK && got != frames) hrc = AMX_EINVAL;
    } else if (hrc == AMX_OK) {
        hrc = AMX_EINVAL;   // an empty stream: nothing to compare
    }
    if (R.status == AMX_EUNSUPPORTED) {
        counts[0]++;
        return 0;
    }
    if (hrc != AMX_OK) {
        // the core never accepts what the host refuses: both read the same checks
        if (R.status == AMX_OK) return 1;
        counts[1]++;
        return 0;
    }
    if (R.status == AMX_OK) {
        if (R.pcm != pcm || R.blocks != blocks) return 1;
        counts[2]++;
        return 0;
    }
    if (!R.width_stop) return 1;
    counts[3]++;
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 5 && !std::strcmp(argv[1], "decode")) {
        std::vector<uint8_t> b;
        if (!read_file(argv[2], b)) return 4;
        Result R = decode_copy(b.data(), b.size());
        if (R.status == AMX_EUNSUPPORTED) return 3;
        if (R.status != AMX_OK) return 2;
        if (!write_file(argv[3], R.pcm.data(), R.pcm.size() * 4) ||
            !write_file(argv[4], R.blocks.data(), R.blocks.size() * 4))
            return 4;
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "fuzz")) {
        std::vector<uint8_t> b;
        if (!read_file(argv[2], b) || b.size() < 8) return 4;
        rng_state = std::strtoull(argv[3], nullptr, 10);
        const int flips = std::atoi(argv[4]), cuts = std::atoi(argv[5]);
        int counts[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < flips + cuts; i++) {
            std::vector<uint8_t> m = b;
            const char *what;
            size_t at;
            if (i < flips) {
                what = "flip";
                at = 4 + (size_t)(rnd() % (b.size() - 4));
                m[at] ^= (uint8_t)(1 + rnd() % 255);
            } else {
                what = "cut";
                at = 4 + (size_t)(rnd() % (b.size() - 4));
                m.resize(at);
            }
            if (compare(m, counts)) {
                std::printf("DISAGREE %s at %zu (case %d)\n", what, at, i);
                return 1;
            }
        }
        std::printf("%d cases: %d unsupported, %d both refuse, %d equal, %d refused for width\n", flips + cuts,
                    counts[0], counts[1], counts[2], counts[3]);
        return 0;
    }
    std::fprintf(stderr, "usage: %s decode IN OUT.i32 OUT.blocks | fuzz IN SEED FLIPS CUTS\n", argv[0]);
    return 4;
}
