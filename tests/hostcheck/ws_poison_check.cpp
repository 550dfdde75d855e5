// ws_poison_check -- the parser of the test hook VO_WS_POISON (visual-odometry_amd/csrc/ws_poison.h) without a GPU and without
// the library: a stand-alone program over the header alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I visual-odometry_amd/csrc
//       tests/hostcheck/ws_poison_check.cpp -o ws_poison_check && ./ws_poison_check      (ends with "ws_poison_check: ok")
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ws_poison.h"

static int g_bad = 0;
#define CHECK(cond) \
  do { if (!(cond)) { ++g_bad; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

int main() {
  // the values the hook's description names
  CHECK(ws_poison_parse(nullptr) == -1);      // unset
  CHECK(ws_poison_parse("") == -1);
  CHECK(ws_poison_parse("0") == 0);
  CHECK(ws_poison_parse("255") == 255);
  CHECK(ws_poison_parse("0xff") == 255);
  CHECK(ws_poison_parse("256") == -1);
  CHECK(ws_poison_parse("-1") == -1);
  CHECK(ws_poison_parse("abc") == -1);
  // and their neighbours
  CHECK(ws_poison_parse("165") == 165 && ws_poison_parse("0xA5") == 165 && ws_poison_parse("0XA5") == 165 && ws_poison_parse("0xa5") == 165);
  CHECK(ws_poison_parse("0x") == -1 && ws_poison_parse("0x100") == -1 && ws_poison_parse("0x0") == 0 && ws_poison_parse("00") == 0);
  CHECK(ws_poison_parse("ff") == -1 && ws_poison_parse("1 ") == -1 && ws_poison_parse(" 1") == -1 && ws_poison_parse("+1") == -1);
  CHECK(ws_poison_parse("1.0") == -1 && ws_poison_parse("0xfg") == -1 && ws_poison_parse("99999999999999999999999") == -1);
  // every byte, both spellings, through a heap copy of exactly the string's length (the sanitizer sees a read past the end)
  for (int v = 0; v < 256; ++v) {
    char buf[16];
    for (int hex = 0; hex < 2; ++hex) {
      std::snprintf(buf, sizeof(buf), hex ? "0x%x" : "%d", v);
      const size_t n = std::strlen(buf) + 1;
      char* s = static_cast<char*>(std::malloc(n));
      std::memcpy(s, buf, n);
      CHECK(ws_poison_parse(s) == v);
      std::free(s);
    }
  }
  // the environment, as DevBuf::ensure reads it: per call
  unsetenv("VO_WS_POISON");
  CHECK(ws_poison_byte() == -1);
  setenv("VO_WS_POISON", "0xA5", 1);
  CHECK(ws_poison_byte() == 165);
  setenv("VO_WS_POISON", "", 1);
  CHECK(ws_poison_byte() == -1);
  setenv("VO_WS_POISON", "256", 1);
  CHECK(ws_poison_byte() == -1);
  unsetenv("VO_WS_POISON");
  CHECK(ws_poison_byte() == -1);
  if (g_bad) { std::printf("ws_poison_check: %d FAILED\n", g_bad); return 1; }
  std::printf("ws_poison_check: ok\n");
  return 0;
}
