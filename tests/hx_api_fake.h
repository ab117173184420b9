// hx_api_fake.h - what tests/hx_api_trace_driver.cpp asks of the fake runtime beside it (tests/hx_api_fake_runtime.cpp)
#pragma once
#include <string>

namespace fake {
void say(const std::string& line);   // a line of the driver's own: whatever was recorded before it is printed first
void flush();                        // prints what is recorded: allocations, frees and synchronous copies between two stream operations sorted
void fail_memcpy(int k);             // the k-th synchronous hipMemcpy from now on fails, once (0: none)
std::string where(const void* p);    // "b<index>+<bytes>" of a device pointer, "host" of any other
}  // namespace fake
