// mph_env.h -- the one way the library reads its MPH_* environment knobs (table: INTEGRATION.md).
// Header-only, no HIP.  A knob's rule is spelled at its one call site from these four:
//   off only at "0"      !env_is(name, "0")          ("00", "no", "" leave it on)
//   on only at 1         env_int(name, 0) == 1       (atoi: "1", "01", "1x")
//   off at a zero number env_int(name, 1) == 0       (atoi: "0", "00", "", "no" -- any text without a number)
#pragma once

#include <cstdlib>
#include <cstring>

namespace mph {

// the value, "" when unset
inline const char* env_str(const char* name)
{
    const char* e = std::getenv(name);
    return e ? e : "";
}

// set, and exactly `value`
inline bool env_is(const char* name, const char* value)
{
    const char* e = std::getenv(name);
    return e && std::strcmp(e, value) == 0;
}

// atoi of the value when set (0 for "" and for text without a leading number), else dflt
inline int env_int(const char* name, int dflt)
{
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

// atof of the value when set, else dflt
inline double env_double(const char* name, double dflt)
{
    const char* e = std::getenv(name);
    return e ? std::atof(e) : dflt;
}

}  // namespace mph
