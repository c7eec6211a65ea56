// Host-only stand-in for the four HIP allocation calls csrc/device_buffer.hpp uses (tests/test_device_buffer_cpu.py):
// the definitions, made of malloc / free and call counters, are in device_buffer_check.cpp.
#pragma once
#include <cstddef>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2;
constexpr unsigned hipHostMallocDefault = 0;

hipError_t hipMalloc(void** p, size_t n);
hipError_t hipFree(void* p);
hipError_t hipHostMalloc(void** p, size_t n, unsigned flags);
hipError_t hipHostFree(void* p);
