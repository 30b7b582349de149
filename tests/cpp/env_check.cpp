// env_check: Env::load() (radix_sorting_amd/csrc/rsx_env.hpp) on the CPU -- what every kind of RSX_* switch parses to, and that a
// variable taken away again gives the default back ON THE SAME OBJECT: rsx_reload_env() between two tests relies on it.
// The expected values are the parse rules as they were before the loader was rewritten; exits non-zero at the first mismatch.
#include "../../radix_sorting_amd/csrc/rsx_env.hpp"

#include <cstdio>

static Env e;   // one object throughout, as the library's g_env

// load() with `name` = `text` (nullptr: absent)
static void load_with(const char *name, const char *text)
{
	if (text)
		setenv(name, text, 1);
	else
		unsetenv(name);
	e.load();
}

#define EXPECT(name, text, field, want)                                                                              \
	do {                                                                                                             \
		load_with(name, text);                                                                                       \
		if ((long long)(e.field) != (long long)(want)) {                                                             \
			fprintf(stderr, "env_check: %s=%s: %s is %lld, expected %lld\n", name, (text) ? (const char *)(text) : "(absent)", #field, \
			        (long long)(e.field), (long long)(want));                                                        \
			return 1;                                                                                                \
		}                                                                                                            \
	} while (0)
// ... and absent again: the field of a fresh Env
#define EXPECT_DEFAULT(name, field) EXPECT(name, nullptr, field, Env{}.field)

int main()
{
	// the three switches that kept their value once set
	EXPECT("RSX_PASS32_MIN_MI", "8", pass32_min_mi, 8);
	EXPECT_DEFAULT("RSX_PASS32_MIN_MI", pass32_min_mi);
	EXPECT("RSX_PASS32_PREFETCH", "1", pass32_prefetch, 1);
	EXPECT_DEFAULT("RSX_PASS32_PREFETCH", pass32_prefetch);
	EXPECT("RSX_PASS32_PREFETCH", "0", pass32_prefetch, 0);
	EXPECT_DEFAULT("RSX_PASS32_PREFETCH", pass32_prefetch);
	EXPECT("RSX_FORCE_LEAFC", "3", force_leafc, 3);
	EXPECT_DEFAULT("RSX_FORCE_LEAFC", force_leafc);
	// "set"
	EXPECT("RSX_NO_HOT", "", no_hot, 1);
	EXPECT("RSX_NO_HOT", "0", no_hot, 1);
	EXPECT_DEFAULT("RSX_NO_HOT", no_hot);
	// "=1": the first character is '1'
	EXPECT("RSX_NO_BLIND", "1", no_blind, 1);
	EXPECT("RSX_NO_BLIND", "0", no_blind, 0);
	EXPECT("RSX_NO_BLIND", "2", no_blind, 0);
	EXPECT("RSX_NO_BLIND", "1", no_blind, 1);
	EXPECT_DEFAULT("RSX_NO_BLIND", no_blind);
	// the first character is '1' or '2'
	EXPECT("RSX_VERIFY", "1", verify, 1);
	EXPECT("RSX_VERIFY", "1", verify_whole, 0);
	EXPECT("RSX_VERIFY", "2", verify, 0);
	EXPECT("RSX_VERIFY", "2", verify_whole, 1);
	EXPECT_DEFAULT("RSX_VERIFY", verify);
	EXPECT_DEFAULT("RSX_VERIFY", verify_whole);
	EXPECT("RSX_TOPK_FORCE", "1", topk_force, 1);
	EXPECT("RSX_TOPK_FORCE", "2", topk_force, 2);
	EXPECT("RSX_TOPK_FORCE", "3", topk_force, 0);
	EXPECT("RSX_TOPK_FORCE", "2", topk_force, 2);
	EXPECT_DEFAULT("RSX_TOPK_FORCE", topk_force);
	// atoi clamped to [lo, hi]
	EXPECT("RSX_BLIND_MIN_LOG2", "5", blind_min_log2, 22);
	EXPECT("RSX_BLIND_MIN_LOG2", "99", blind_min_log2, 30);
	EXPECT_DEFAULT("RSX_BLIND_MIN_LOG2", blind_min_log2);
	EXPECT("RSX_LEAF_GRID", "1", leaf_grid, 256);
	EXPECT("RSX_LEAF_GRID", "999999", leaf_grid, 65536);
	EXPECT("RSX_LEAF_GRID", "1", leaf_grid, 256);
	EXPECT_DEFAULT("RSX_LEAF_GRID", leaf_grid);
	EXPECT("RSX_UNIQUE_MAX_BITS", "31", unique_max_bits, 30);
	EXPECT_DEFAULT("RSX_UNIQUE_MAX_BITS", unique_max_bits);
	// atoi taken only inside [lo, hi], else the default
	EXPECT("RSX_TWO_LEVEL_MIN_LOG2", "21", two_level_min_log2, 27);
	EXPECT("RSX_TWO_LEVEL_MIN_LOG2", "31", two_level_min_log2, 27);
	EXPECT("RSX_TWO_LEVEL_MIN_LOG2", "22", two_level_min_log2, 22);
	EXPECT_DEFAULT("RSX_TWO_LEVEL_MIN_LOG2", two_level_min_log2);
	EXPECT("RSX_LEX_PACK_BYTES", "0", lex_pack_bytes, LEX_PACK_BYTES_DEFAULT);
	EXPECT("RSX_LEX_PACK_BYTES", "9", lex_pack_bytes, LEX_PACK_BYTES_DEFAULT);
	EXPECT("RSX_LEX_PACK_BYTES", "8", lex_pack_bytes, 8);
	EXPECT_DEFAULT("RSX_LEX_PACK_BYTES", lex_pack_bytes);
	// 1 -> 1, anything else -> 2
	EXPECT("RSX_PASS16_WGS", "1", pass16_wgs, 1);
	EXPECT("RSX_PASS16_WGS", "7", pass16_wgs, 2);
	EXPECT("RSX_PASS16_WGS", "1", pass16_wgs, 1);
	EXPECT_DEFAULT("RSX_PASS16_WGS", pass16_wgs);
	// the defaults the comments in rsx_env.hpp and rsx.h name, after all of the above on the same object
	Env fresh;
	if (fresh.pass32_min_mi != 0 || fresh.pass32_prefetch != -1 || fresh.force_leafc != 0 || fresh.two_level_min_log2 != 27 ||
	    fresh.leaf_grid != 65536 || fresh.pass16_wgs != 2 || fresh.unique_max_bits != UNIQUE_MAX_BITS_DEFAULT) {
		fprintf(stderr, "env_check: a default initialiser of Env has changed\n");
		return 1;
	}
	(void)g_env_epoch.load();
	(void)env();
	printf("env_check OK\n");
	return 0;
}
