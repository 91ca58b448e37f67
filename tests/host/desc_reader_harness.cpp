// desc_reader_harness.cpp -- the renderer's proto reader (video_segment_amd/render/render_desc.h) on its own,
// for tests/test_desc_reader.py: no device, no HIP call.  Built with the host sanitizers; every input is parsed
// from a heap block of exactly its size, so that a read past its end is reported.
//
//   desc_reader_harness sweep FILE W H INSIDE IDS INTERVALS HIERARCHY LINES
//     FILE parsed for a W x H frame has to give the region ids IDS, INTERVALS scan intervals per region, the
//     hierarchy level sizes HIERARCHY (comma lists; "-": empty) and LINES polygon lines (-1: not vector-only).
//     Then every prefix of it and every replacement of one byte by 0x00, 0x7f, 0x80 and 0xff: each has to
//     parse or to be refused as VSG_ERR_INVALID.  The empty prefix has to parse, the prefix of INSIDE bytes,
//     which ends inside a length-delimited payload, has to be refused.  Prints the counts of both outcomes.
//   desc_reader_harness one FILE W H
//     FILE alone: parses or is refused as VSG_ERR_INVALID.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/vsg_render.h"
#include "../../video_segment_amd/render/render.h"
#include "../../video_segment_amd/common/capi_support.h"
#include "../../video_segment_amd/render/render_desc.h"

namespace {

struct Parsed {
  bool vector = false;
  ParsedDesc desc;
  std::vector<Interval> intervals;
  std::vector<float> scaled_mesh;
  std::vector<VecLine> lines;
  int64_t crossings = 0;
};

// What the library does with a desc before any device work, in its order.
int Parse(const std::vector<uint8_t>& bytes, int W, int H, Parsed* out) {
  // a block of its own, exactly as long as the input
  const std::vector<uint8_t> seg(bytes.begin(), bytes.end());
  return Guard([&] {
    out->vector = IsVectorOnly(seg.data(), seg.size());
    ParseDesc(seg.data(), seg.size(), W, H, out->vector, &out->desc, &out->intervals);
    const Hierarchy& hier = out->desc.hierarchy;
    for (int level = 0; level < (int)std::max<size_t>(hier.size(), 1); ++level) {
      for (int32_t id : out->desc.region_ids) (void)ParentId(id, level, hier);
    }
    out->lines.clear();
    if (out->vector) out->crossings = BuildLines(out->desc, W, H, &out->scaled_mesh, &out->lines);
  });
}

[[noreturn]] void Fail(const std::string& what) {
  std::fprintf(stderr, "desc_reader_harness: %s\n", what.c_str());
  std::exit(1);
}

// Parses or is refused as invalid; anything else ends the run.  Returns whether it parsed.
bool ParsesOrInvalid(const std::vector<uint8_t>& bytes, int W, int H, const std::string& what) {
  Parsed p;
  const int rc = Parse(bytes, W, H, &p);
  if (rc != VSG_OK && rc != VSG_ERR_INVALID) {
    Fail(what + ": status " + std::to_string(rc) + " (" + g_last_error + ")");
  }
  return rc == VSG_OK;
}

std::vector<long long> List(const std::string& text) {
  std::vector<long long> out;
  if (text == "-") return out;
  std::stringstream in(text);
  std::string item;
  while (std::getline(in, item, ',')) out.push_back(std::stoll(item));
  return out;
}

std::string Text(const std::vector<long long>& v) {
  std::string s;
  for (long long x : v) s += (s.empty() ? "" : ",") + std::to_string(x);
  return s.empty() ? "-" : s;
}

void Expect(const char* what, const std::vector<long long>& got, const std::vector<long long>& want) {
  if (got != want) Fail(std::string("intact: ") + what + " " + Text(got) + ", expected " + Text(want));
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (!((mode == "sweep" && argc == 10) || (mode == "one" && argc == 5))) Fail("bad arguments");
  std::ifstream file(argv[2], std::ios::binary);
  if (!file) Fail(std::string("cannot read ") + argv[2]);
  const std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
  if (mode == "one") {
    std::printf("one: %s\n", ParsesOrInvalid(bytes, W, H, "the input") ? "parsed" : "rejected");
    return 0;
  }

  // ---- the desc as it is ----
  Parsed p;
  const int rc = Parse(bytes, W, H, &p);
  if (rc != VSG_OK) Fail("intact: status " + std::to_string(rc) + " (" + g_last_error + ")");
  std::vector<long long> ids(p.desc.region_ids.begin(), p.desc.region_ids.end()), counts, levels;
  for (size_t r = 0; r + 1 < p.desc.region_begin.size(); ++r) {
    counts.push_back((long long)(p.desc.region_begin[r + 1] - p.desc.region_begin[r]));
  }
  for (const std::vector<CompoundRef>& level : p.desc.hierarchy) levels.push_back((long long)level.size());
  Expect("region ids", ids, List(argv[6]));
  Expect("intervals per region", counts, List(argv[7]));
  Expect("hierarchy level sizes", levels, List(argv[8]));
  Expect("polygon lines", {p.vector ? (long long)p.lines.size() : -1}, {std::atoll(argv[9])});
  std::printf("intact: regions=%zu intervals=%zu levels=%zu vector=%d lines=%zu crossings=%lld\n", ids.size(),
              p.intervals.size(), levels.size(), p.vector ? 1 : 0, p.lines.size(), (long long)p.crossings);

  // ---- every prefix ----
  const size_t inside = (size_t)std::atoll(argv[5]);
  size_t parsed = 0, rejected = 0;
  for (size_t n = 0; n <= bytes.size(); ++n) {
    const std::vector<uint8_t> prefix(bytes.begin(), bytes.begin() + n);
    const bool ok = ParsesOrInvalid(prefix, W, H, "the prefix of " + std::to_string(n) + " bytes");
    if (n == 0 && !ok) Fail("the empty prefix was refused: " + g_last_error);
    if (n == inside && ok) Fail("the prefix of " + std::to_string(n) + " bytes ends inside a payload and parsed");
    ++(ok ? parsed : rejected);
  }
  std::printf("prefixes: parsed=%zu rejected=%zu\n", parsed, rejected);

  // ---- every byte replaced ----
  parsed = rejected = 0;
  std::vector<uint8_t> changed = bytes;
  for (size_t at = 0; at < bytes.size(); ++at) {
    for (const uint8_t value : {0x00, 0x7f, 0x80, 0xff}) {
      if (value == bytes[at]) continue;
      changed[at] = value;
      ++(ParsesOrInvalid(changed, W, H, "byte " + std::to_string(at) + " set to " + std::to_string(value)) ? parsed
                                                                                                          : rejected);
    }
    changed[at] = bytes[at];
  }
  std::printf("mutations: parsed=%zu rejected=%zu\n", parsed, rejected);
  return 0;
}
