// The one place where libaprilasr reads its environment.  Every name read through these two functions is listed, with its
// default and meaning, in the "Environment" table of INTEGRATION.md (tests/test_env_names.py holds the two lists together).
#pragma once
#include <cstdlib>

namespace aprilx {

// value of `name`, or nullptr when it is unset or empty
inline const char *env_str(const char *name) { const char *v = getenv(name); return v && *v ? v : nullptr; }
inline int env_int(const char *name, int def) { const char *v = env_str(name); return v ? atoi(v) : def; }

}  // namespace aprilx
