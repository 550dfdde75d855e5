// ws_poison.h -- the test hook VO_WS_POISON ("The workspace contract"): the byte DevBuf::ensure fills a workspace
// with before the call that sized it runs.  Plain C++, no HIP include: tests/hostcheck/ws_poison_check.cpp compiles it alone.
#pragma once

#include <cstdlib>

// the value of VO_WS_POISON as text: 0 .. 255, decimal ("165") or hexadecimal ("0xa5", "0XA5"); -1 (off) for a null pointer,
// the empty string, a sign, a blank, any other character, or a value above 255
inline int ws_poison_parse(const char* s) {
  if (!s || !s[0]) return -1;
  int base = 10;
  if (s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) { base = 16; s += 2; if (!s[0]) return -1; }
  int v = 0;
  for (; *s; ++s) {
    int d;
    if (*s >= '0' && *s <= '9') d = *s - '0';
    else if (base == 16 && *s >= 'a' && *s <= 'f') d = *s - 'a' + 10;
    else if (base == 16 && *s >= 'A' && *s <= 'F') d = *s - 'A' + 10;
    else return -1;
    v = v * base + d;
    if (v > 255) return -1;
  }
  return v;
}

// read per call, like the library's other test hooks: a test flips it in-process
inline int ws_poison_byte() { return ws_poison_parse(getenv("VO_WS_POISON")); }
