// File helpers of the host rules programs (tests/*_rules.cpp, tests/edit_record_rule.cpp).  Nothing of the library: the programs that are also
// built without it (lift_rules, shape_rules) include this header alone; the ones that read worlds include tests/rules_world.h, which brings it in.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// The whole file; a file that cannot be opened ends the program with exit code 2.
static std::vector<uint8_t> ReadFile(const char *path)
{
	std::vector<uint8_t> out;
	FILE *f = std::fopen(path, "rb");
	if (!f) { std::exit(2); }
	uint8_t buffer[65536];
	for (size_t got; (got = std::fread(buffer, 1, sizeof buffer, f)) > 0;) { out.insert(out.end(), buffer, buffer + got); }
	std::fclose(f);
	return out;
}

// The file as whole T's (a partial one at the end is dropped), aligned for T.
template <class T>
static std::vector<T> ReadWords(const char *path)
{
	const std::vector<uint8_t> raw = ReadFile(path);
	std::vector<T> out(raw.size() / sizeof(T));
	if (!out.empty()) { std::memcpy(out.data(), raw.data(), out.size() * sizeof(T)); }
	return out;
}

// 0, or 2 when the file cannot be made: what the program returns.
static int WriteFile(const char *path, const void *data, size_t bytes)
{
	FILE *f = std::fopen(path, "wb");
	if (!f) { return 2; }
	std::fwrite(data, 1, bytes, f);
	std::fclose(f);
	return 0;
}

template <class T>
static int WriteFile(const char *path, const std::vector<T> &out)
{
	return WriteFile(path, out.data(), out.size() * sizeof(T));
}
