// bring-up (gpu_tally.py): what a caller does today with the cut's packed text once it is on the host: one core, one
// std::unordered_map<std::string_view, uint64_t> over the records, the keys kept in order of first appearance. The rules are
// ZraHipTallyRecords': bytes behind the last delimiter form one more record iff there are any; a record longer than maxKey is skipped.
// Build: c++ -O2 -std=c++17 -shared -fPIC host_tally.cpp -o host_tally.so
#include <cstdint>
#include <string_view>
#include <unordered_map>
#include <vector>

extern "C" uint64_t host_tally(const char* text, uint64_t n, char delimiter, uint64_t maxKey, uint64_t* entries, uint64_t cap, uint64_t* nRecords, uint64_t* nSkipped) {
  std::unordered_map<std::string_view, uint64_t> index;                      // key -> its entry
  std::vector<uint64_t> out;                                                 // {offset, size, count} per entry
  uint64_t records = 0, skipped = 0;
  for (uint64_t at = 0; at < n;) {
    uint64_t end = at;
    while (end < n && text[end] != delimiter) end++;
    records++;
    if (end - at > maxKey) skipped++;
    else {
      auto [it, fresh] = index.try_emplace(std::string_view(text + at, end - at), out.size() / 3);
      if (fresh) { out.push_back(at); out.push_back(end - at); out.push_back(1); }
      else out[3 * it->second + 2]++;
    }
    at = end + 1;
  }
  *nRecords = records; *nSkipped = skipped;
  for (uint64_t i = 0; i < out.size() && i < 3 * cap; i++) entries[i] = out[i];
  return out.size() / 3;
}
