// What the stand-alone drivers of the entries' host side (*_args_main.cpp, built and run by `make asan-<name>` against the
// AddressSanitizer build of the library) share: the failure count, the check of a refusal and the final line.
#pragma once
#include <stdio.h>
#include <string.h>

#include "../../include/nesti_hip.h"

static int failures = 0;

// the call was refused (rc != 0) and the message names `word`
static void refused(int rc, const char* word, const char* what) {
  const char* msg = nesti_last_error();
  if (rc == 0 || !msg || !strstr(msg, word)) {
    printf("FAIL %s: rc %d, message '%s'\n", what, rc, msg ? msg : "(null)");
    ++failures;
  }
}

// prints "<name>: ok" or the number of failures; the value main() returns
static int finish(const char* name) {
  if (failures) printf("%s: %d failure(s)\n", name, failures);
  else printf("%s: ok\n", name);
  return failures ? 1 : 0;
}
