// The PNG decoder's code (swem_amd/csrc/inflate_core.h: chunk walk, bit reader, code tables, symbol decode, inflate, Adler-32,
// unfilter, unpack) run on the host: the 64 lanes of png_decode_kernel (csrc/png_decode.hip) as a loop, its barrier as nothing.
// tests/test_png_decode_host.py compiles this as ordinary C++ -- also under AddressSanitizer, with every buffer allocated at
// exactly the size the C ABI promises the kernel -- and compares with the strict readers; tests/test_gpu_png_decode.py compares
// the device's results with these byte for byte.
//   png_decode_host batch.bin T Hs Ws channels out_prefix
//     batch.bin  : T + 1 little-endian int64 offsets, then the blob they index (as swem_png_decode_u8 takes them)
//     -> out_prefix.pixels [T][Hs][Ws][channels], .sizes [T][2] int32, .palettes [T][768], .npal [T] int32, .status [T] int32
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "inflate_core.h"

typedef unsigned char u8;

struct HostLanes {
  int lane_begin() const { return 0; }
  int lane_end() const { return 64; }
  bool first() const { return true; }
  void sync() const {}
};

template <class V>
static bool put(const char *prefix, const char *ext, const V &v) {
  char name[4096];
  snprintf(name, sizeof name, "%s.%s", prefix, ext);
  FILE *fp = fopen(name, "wb");
  if (!fp) return false;
  const size_t bytes = v.size() * sizeof(v[0]);
  const bool ok = fwrite(v.data(), 1, bytes, fp) == bytes;
  return fclose(fp) == 0 && ok;
}

int main(int argc, char **argv) {
  if (argc != 7) return 2;
  const int T = atoi(argv[2]), Hs = atoi(argv[3]), Ws = atoi(argv[4]), channels = atoi(argv[5]);
  if (T < 1 || Hs < 1 || Ws < 1 || (channels != 1 && channels != 3) || (long long)channels * Ws + 1 > 65535 ||
      (long long)Hs * ((long long)channels * Ws + 1) >= 0x80000000ll)
    return 2;
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) return 3;
  std::vector<long long> offsets(T + 1);
  if (fread(offsets.data(), sizeof(long long), T + 1, fp) != (size_t)T + 1) return 3;
  const long at = ftell(fp);
  fseek(fp, 0, SEEK_END);
  const size_t blob_bytes = (size_t)(ftell(fp) - at);
  fseek(fp, at, SEEK_SET);
  std::vector<u8> blob(blob_bytes);
  if (blob_bytes < 1 || fread(blob.data(), 1, blob_bytes, fp) != blob_bytes) return 3;
  fclose(fp);

  const size_t slot = (size_t)Hs * Ws * channels, raw_cap = (size_t)Hs * ((size_t)channels * Ws + 1);
  std::vector<u8> pixels(T * slot, 0xA5), palettes((size_t)T * 768, 0xA5);
  std::vector<int> sizes(2 * (size_t)T, -1), npal(T, -1), status(T, -1);
  static PngdLds S;
  const HostLanes wv;
  for (int t = 0; t < T; ++t) {
    // this file's parts of the workspace, each an allocation of its own: the sanitizer sees a byte past either.  The compacted
    // stream sits at comp_ws + offsets[t] and takes the file's length (nothing, when the offsets are refused).
    const long long o0 = offsets[t], o1 = offsets[t + 1];
    const bool ok = o0 >= 0 && o1 >= o0 && (unsigned long long)o1 <= blob_bytes;
    std::vector<u8> comp(ok ? (size_t)(o1 - o0) : 0, 0xA5), raw(raw_cap, 0xA5);
    // a file's neighbours in the blob would hide a read past offsets[t + 1]: a file whose offsets hold is handed a copy of its
    // own bytes as a blob of its own, so that such a read is a read past an allocation
    std::vector<u8> mine(ok ? blob.begin() + o0 : blob.begin(), ok ? blob.begin() + o1 : blob.begin());
    if (ok)
      pngd_decode_file(wv, &S, mine.data(), mine.size(), 0, (long long)mine.size(), Hs, Ws, channels, pixels.data() + t * slot,
                       &sizes[2 * t], &palettes[(size_t)t * 768], &npal[t], &status[t], comp.data(), raw.data(), (uint32_t)raw_cap);
    else
      pngd_decode_file(wv, &S, blob.data(), blob_bytes, o0, o1, Hs, Ws, channels, pixels.data() + t * slot, &sizes[2 * t],
                       &palettes[(size_t)t * 768], &npal[t], &status[t], (u8 *)nullptr, raw.data(), (uint32_t)raw_cap);
  }
  if (!put(argv[6], "pixels", pixels) || !put(argv[6], "sizes", sizes) || !put(argv[6], "palettes", palettes) ||
      !put(argv[6], "npal", npal) || !put(argv[6], "status", status))
    return 4;
  return 0;
}
