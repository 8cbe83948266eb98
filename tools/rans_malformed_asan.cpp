// Malformed rans1 streams through the host twin under AddressSanitizer / UBSan (host code only):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include -I cnc_amd/csrc \
//       tools/rans_malformed_asan.cpp cnc_amd/csrc/rans_coder.cpp -o /tmp/rans_asan && /tmp/rans_asan
// Every buffer is a heap allocation of exactly the size handed to the library, so a read past in[len) or a write past
// x_out[n) is a report, not luck.  The cases are those of tests/test_rans_twin.py plus a sweep that damages every byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cnc_codec.h"

static int run(const std::vector<float>& p, int64_t n, const std::vector<uint8_t>& s, int64_t* k_out)
{
    uint8_t* in = static_cast<uint8_t*>(malloc(s.size() ? s.size() : 1));       // exact size: the redzone starts at len
    if (!s.empty()) memcpy(in, s.data(), s.size());
    float* x = static_cast<float*>(malloc(sizeof(float) * (n ? n : 1)));
    *k_out = cnc_rans_check(in, static_cast<int64_t>(s.size()), n);
    const int rc = cnc_rans_decode_pm1_host(p.data(), 1, n, in, static_cast<int64_t>(s.size()), x);
    free(x);
    free(in);
    return rc;
}

int main()
{
    const int64_t n = 1029, S = 16;
    std::vector<float> p(n), x(n);
    uint32_t lcg = 12345u;
    auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (lcg >> 8) * (1.0f / 16777216.0f); };
    for (int64_t i = 0; i < n; ++i) {
        p[i] = 0.02f + 0.96f * rnd();
        x[i] = rnd() < p[i] ? 1.0f : -1.0f;
    }
    std::vector<uint8_t> good(static_cast<size_t>(cnc_rans_bound(n, S)));
    const int64_t len = cnc_rans_encode_pm1_host(p.data(), 1, x.data(), n, S, good.data(), static_cast<int64_t>(good.size()));
    if (len <= 0) return 1;
    good.resize(static_cast<size_t>(len));
    const int64_t K = (n + S - 1) / S, w = good[1];
    int64_t k = 0;
    int failures = 0;
    auto expect = [&](const char* name, const std::vector<uint8_t>& s, bool check_fails) {
        const int rc = run(p, n, s, &k);
        const bool ok = check_fails ? (k == -3 && rc == -3) : (k == K && (rc == 0 || rc == -3));
        printf("%-28s check %4lld decode %2d %s\n", name, static_cast<long long>(k), rc, ok ? "ok" : "UNEXPECTED");
        failures += !ok;
    };
    expect("well-formed", good, false);
    expect("truncated", std::vector<uint8_t>(good.begin(), good.end() - 5), true);
    expect("truncated in directory", std::vector<uint8_t>(good.begin(), good.begin() + 6 + K / 2), true);
    expect("header only", std::vector<uint8_t>(good.begin(), good.begin() + 6), true);
    expect("empty", std::vector<uint8_t>(), true);
    auto v = good;
    v[6 + 3 * w] = 0xFF;
    expect("directory sum > len", v, true);
    v = good;
    v[2] = static_cast<uint8_t>((n + 1) & 0xFF);
    v[3] = static_cast<uint8_t>((n + 1) >> 8);
    expect("K > n", v, true);
    v = good;
    v[2] = v[3] = v[4] = v[5] = 0xFF;
    expect("K = 2^32 - 1", v, true);
    v = good;
    v[good.size() / 2] ^= 0x10;
    expect("flipped payload byte", v, false);
    v = good;
    v[6] += 1;
    v[6 + w] -= 1;
    expect("directory shifted", v, false);
    // every byte of the stream damaged in turn, and every truncation: any outcome but a memory error
    for (size_t at = 0; at < good.size(); ++at) {
        v = good;
        v[at] ^= 0xFF;
        run(p, n, v, &k);
    }
    for (size_t cut = 0; cut < good.size(); cut += 7) run(p, n, std::vector<uint8_t>(good.begin(), good.begin() + cut), &k);
    printf("sweeps done; %d unexpected\n", failures);
    return failures != 0;
}
