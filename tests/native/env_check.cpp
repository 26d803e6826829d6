// What the helpers of csrc/mph_env.h return for the value of MPH_T in this process's environment
// (tests/test_env_knobs.py runs it once per value).
#include <cstdio>

#include "mph_env.h"

int main()
{
    using namespace mph;
    std::printf("int0=%d int1=%d dbl=%g is0=%d is1=%d isauto=%d isempty=%d str=[%s]\n", env_int("MPH_T", 0),
                env_int("MPH_T", 1), env_double("MPH_T", 0.25), (int)env_is("MPH_T", "0"), (int)env_is("MPH_T", "1"),
                (int)env_is("MPH_T", "auto"), (int)env_is("MPH_T", ""), env_str("MPH_T"));
    return 0;
}
