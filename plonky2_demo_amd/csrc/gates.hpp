// The gate set: the ONE place that says which gates exist and what shape each has.  Host and device code; everything here is usable
// in a constant expression.  A new gate is a row of GATE_TABLE (plus its name in GL_GATE_LIST, checked below), its constraint body in
// prover_kernels.cuh and its case in verifier.hip's gate_constraints_at; the serialiser, the gate-order check, the launch selection and
// the table sizes follow the row.
#pragma once
#include <stdint.h>
#include "gl64.cuh"
#include "../../include/plonky2_mi355x.h"

namespace glhost {

// gate type codes of gl_circuit_desc.gate_types, shared with the device kernels (ABI: the values never change)
enum { G_NOOP = 0, G_CONSTANT = 1, G_PUBLIC_INPUT = 2, G_ARITHMETIC = 3, G_POSEIDON = 4, G_BASE_SUM = 5, G_LOOKUP = 6, G_LOOKUP_TABLE = 7, G_EXPONENTIATION = 8,
       G_RANDOM_ACCESS = 9, G_ARITHMETIC_EXT = 10, G_MUL_EXT = 11, G_REDUCING = 12, G_REDUCING_EXT = 13, G_LAST = G_REDUCING_EXT };

// ---- the new_from_config parameters under standard_recursion_config (D = 2, 80 routed wires, 135 wires, 2 constants) ----
// ArithmeticGate num_ops = 80 / 4 (gates/arithmetic_base.rs:35-38), ConstantGate num_consts = config.num_constants (circuit_data.rs:78)
enum { ARITH_OPS = 20, STD_NUM_CONSTANTS = 2 };
// ArithmeticExtensionGate num_ops = 80 / 8 (gates/arithmetic_extension.rs:35-38), MulExtensionGate num_ops = 80 / 6
// (gates/multiplication_extension.rs:35-38), ReducingGate num_coeffs = min(80 - 6, (135 - 4) / 3) (gates/reducing.rs:29-31),
// ReducingExtensionGate num_coeffs = min((80 - 6) / 2, (135 - 4) / 4) (gates/reducing_extension.rs:29-33)
enum { ARITH_EXT_OPS = 10, MUL_EXT_OPS = 13, REDUCING_COEFFS = 43, REDUCING_EXT_COEFFS = 32 };
// ExponentiationGate::new_from_config (gates/exponentiation.rs:43-53): min(routed - 2, (wires - 2) / 2) = 66 power bits; wires: 0 base,
// 1..66 power bits (little-endian), 67 output, 68..133 intermediate values; 67 constraints of degree 4
enum { EXP_POWER_BITS = 66 };
enum { LOOKUP_SLOTS = 40, LOOKUP_TABLE_SLOTS = 26 };      // gates/lookup.rs:41-44, gates/lookup_table.rs:47-50
enum { BASE_SUM_LIMBS = 63 };      // BaseSumGate::<2>::new_from_config (gates/base_sum.rs:31-35): wire 0 = sum, wires 1..=63 = limbs
// RandomAccessGate::new_from_config(standard_recursion_config, bits) (gates/random_access.rs:55-110), bits = gate_params[g] in 1..6: copy c
// owns wires (2 + 2^bits) c ..: access index, claimed element, the list; then the extra constants; then (unrouted) every copy's index bits
enum { RANDOM_ACCESS_MIN_BITS = 1, RANDOM_ACCESS_MAX_BITS = 6 };
GL_HD constexpr uint32_t random_access_copies(uint32_t bits) {
    const uint32_t vec_size = 1u << bits, by_routed = 80u / (2u + vec_size), by_wires = 135u / (2u + vec_size + bits);
    return by_routed < by_wires ? by_routed : by_wires;
}
GL_HD constexpr uint32_t random_access_extra_constants(uint32_t bits) {
    const uint32_t left = 80u - (2u + (1u << bits)) * random_access_copies(bits);
    return left < 2u ? left : 2u;
}
GL_HD constexpr uint32_t random_access_constraints(uint32_t bits) { return random_access_copies(bits) * (bits + 2u) + random_access_extra_constants(bits); }      // random_access.rs:285-288
struct RandomAccessLayout {
    uint32_t bits, vec_size, num_copies, num_extra_constants;
    GL_HD explicit RandomAccessLayout(uint32_t b) : bits(b), vec_size(1u << b) {
        num_copies = random_access_copies(b);
        num_extra_constants = random_access_extra_constants(b);
    }
    GL_HD uint32_t wire_access_index(uint32_t c) const { return (2u + vec_size) * c; }
    GL_HD uint32_t wire_claimed_element(uint32_t c) const { return (2u + vec_size) * c + 1u; }
    GL_HD uint32_t wire_list_item(uint32_t i, uint32_t c) const { return (2u + vec_size) * c + 2u + i; }
    GL_HD uint32_t wire_extra_constant(uint32_t i) const { return (2u + vec_size) * num_copies + i; }
    GL_HD uint32_t wire_bit(uint32_t i, uint32_t c) const { return (2u + vec_size) * num_copies + num_extra_constants + c * bits + i; }
    GL_HD uint32_t num_constraints() const { return random_access_constraints(bits); }
};
// PoseidonGate wire layout (gates/poseidon.rs:36-96); 123 constraints (gates/poseidon.rs:403-409): the swap bit, 4 deltas, the S-box
// inputs of 3 + 4 full rounds and 22 partial rounds, 12 outputs
enum { PW_INPUT = 0, PW_OUTPUT = 12, PW_SWAP = 24, PW_DELTA = 25, PW_FULL0 = 29, PW_PARTIAL = 65, PW_FULL1 = 87, PW_END = 135 };
enum { POSEIDON_GATE_CONSTRAINTS = 1 + 4 + 12 * 3 + 22 + 12 * 4 + 12 };

// ---- the table ----
// which quotient launch evaluates a gate's constraints (prover_kernels.cuh): k_quotient<false>, k_quotient<true>, k_quotient_random_access,
// k_quotient_ext_arith; none for the gates without main-trace constraints (gates/lookup.rs:72-75: the lookup argument has its own launch).
// k_quotient<false> always runs (it also holds the permutation terms) and walks every gate that is not the Poseidon launch's; the other
// three are launched when the circuit has a gate of theirs (commit_quotient)
enum GateLaunch : uint8_t { LAUNCH_NONE, LAUNCH_MAIN, LAUNCH_POSEIDON, LAUNCH_RANDOM_ACCESS, LAUNCH_EXT_ARITH };
// what a gate writes behind its tag (write_gate: each gate's serialize()), all usize:
//   WORDS_COUNT        one word, `count`: the only value accepted on reading
//   WORDS_CONFIG_COUNT one word that follows from the circuit config, not from this library (ArithmeticGate num_ops = routed wires / 4,
//                      ConstantGate num_consts): the serialiser derives it from the description and checks it against the config
//   WORDS_RANDOM_ACCESS  bits, num_copies, num_extra_constants (random_access.rs:123-128): bits 1..6, the rest as RandomAccessLayout
//   WORDS_LOOKUP       num_slots = `count`, the table (lookup.rs:59-62);  WORDS_LOOKUP_TABLE: the same, then last_lut_row (lookup_table.rs:70-74)
enum GateWords : uint8_t { WORDS_NONE, WORDS_COUNT, WORDS_CONFIG_COUNT, WORDS_RANDOM_ACCESS, WORDS_LOOKUP, WORDS_LOOKUP_TABLE };
// a row: `type` its own index; `id_name` the leading type name of id() (the Debug string), by which gates of equal degree sort
// (circuit_builder.rs:987); `tag` the position in DefaultGateSerializer's list (util/serialization/gate_serialization.rs:89-107); degree()
// and num_constraints() (the RandomAccessGate's follow from its bits: gate_degree, gate_num_constraints); `refusal` the reader's message
// for a WORDS_COUNT / WORDS_LOOKUP* count other than `count` (null for the other kinds)
struct GateRow {
    uint8_t type; const char* id_name; uint32_t tag; uint8_t degree, constraints;
    GateLaunch launch; GateWords words; uint32_t count; const char* refusal;
};
#define GL_GATE_LIST "{Noop, Constant, PublicInput, Arithmetic, Poseidon, BaseSum<2>, Lookup, LookupTable, Exponentiation, RandomAccess, ArithmeticExtension, MulExtension, Reducing, ReducingExtension}"
#define GL_EXT_COUNT_REFUSAL "ArithmeticExtensionGate / MulExtensionGate / ReducingGate / ReducingExtensionGate with a count other than new_from_config's 10 / 13 / 43 / 32"
#define GL_LOOKUP_REFUSAL "lookup gate: slot count of standard_recursion_config and a table of at most 1024 entries"
static constexpr GateRow GATE_TABLE[] = {
    // type             id_name                    tag deg constraints              launch                words               count                refusal
    {G_NOOP,            "NoopGate",                 9, 0, 0,                         LAUNCH_NONE,          WORDS_NONE,          0,                   nullptr},
    {G_CONSTANT,        "ConstantGate",             3, 1, STD_NUM_CONSTANTS,         LAUNCH_MAIN,          WORDS_CONFIG_COUNT,  STD_NUM_CONSTANTS,   nullptr},      // constant.rs:49-66
    {G_PUBLIC_INPUT,    "PublicInputGate",         12, 1, 4,                         LAUNCH_MAIN,          WORDS_NONE,          0,                   nullptr},      // public_input.rs:44-49
    {G_ARITHMETIC,      "ArithmeticGate",           0, 3, ARITH_OPS,                 LAUNCH_MAIN,          WORDS_CONFIG_COUNT,  ARITH_OPS,           nullptr},      // arithmetic_base.rs:63-92
    {G_POSEIDON,        "PoseidonGate",            11, 7, POSEIDON_GATE_CONSTRAINTS, LAUNCH_POSEIDON,      WORDS_NONE,          0,                   nullptr},
    {G_BASE_SUM,        "BaseSumGate",              2, 2, 1 + BASE_SUM_LIMBS,        LAUNCH_MAIN,          WORDS_COUNT,         BASE_SUM_LIMBS,      "BaseSumGate<2> with a limb count other than new_from_config's 63"},      // base_sum.rs:53-55,144-146
    {G_LOOKUP,          "LookupGate",               6, 0, 0,                         LAUNCH_NONE,          WORDS_LOOKUP,        LOOKUP_SLOTS,        GL_LOOKUP_REFUSAL},
    {G_LOOKUP_TABLE,    "LookupTableGate",          7, 0, 0,                         LAUNCH_NONE,          WORDS_LOOKUP_TABLE,  LOOKUP_TABLE_SLOTS,  GL_LOOKUP_REFUSAL},
    {G_EXPONENTIATION,  "ExponentiationGate",       5, 4, EXP_POWER_BITS + 1,        LAUNCH_MAIN,          WORDS_COUNT,         EXP_POWER_BITS,      "ExponentiationGate with a bit count other than new_from_config's 66"},      // exponentiation.rs:79-81,190-192
    {G_RANDOM_ACCESS,   "RandomAccessGate",        13, 0, 0,                         LAUNCH_RANDOM_ACCESS, WORDS_RANDOM_ACCESS, 0,                   nullptr},
    {G_ARITHMETIC_EXT,  "ArithmeticExtensionGate",  1, 3, 2 * ARITH_EXT_OPS,         LAUNCH_EXT_ARITH,     WORDS_COUNT,         ARITH_EXT_OPS,       GL_EXT_COUNT_REFUSAL},      // arithmetic_extension.rs:59-61,162-164
    {G_MUL_EXT,         "MulExtensionGate",         8, 3, 2 * MUL_EXT_OPS,           LAUNCH_EXT_ARITH,     WORDS_COUNT,         MUL_EXT_OPS,         GL_EXT_COUNT_REFUSAL},      // multiplication_extension.rs:56-58,149-151
    {G_REDUCING,        "ReducingGate",            15, 2, 2 * REDUCING_COEFFS,       LAUNCH_EXT_ARITH,     WORDS_COUNT,         REDUCING_COEFFS,     GL_EXT_COUNT_REFUSAL},      // reducing.rs:63-66,175-177
    {G_REDUCING_EXT,    "ReducingExtensionGate",   14, 2, 2 * REDUCING_EXT_COEFFS,   LAUNCH_EXT_ARITH,     WORDS_COUNT,         REDUCING_EXT_COEFFS, GL_EXT_COUNT_REFUSAL},      // reducing_extension.rs:66-69,175-177
};
static_assert(sizeof GATE_TABLE / sizeof GATE_TABLE[0] == G_LAST + 1, "one row per gate type");

// ---- reading the table ----
inline constexpr const GateRow& gate_row(uint8_t type) { return GATE_TABLE[type]; }      // host / constant expressions; type <= G_LAST
inline constexpr unsigned gate_degree(uint8_t type, uint8_t param) { return type > G_LAST ? 0u : type == G_RANDOM_ACCESS ? param + 1u : GATE_TABLE[type].degree; }
inline constexpr unsigned gate_num_constraints(uint8_t type, uint8_t param) {
    return type > G_LAST ? 0u : type == G_RANDOM_ACCESS ? random_access_constraints(param) : GATE_TABLE[type].constraints;
}
inline constexpr const char* gate_id_name(uint8_t type) { return type <= G_LAST ? GATE_TABLE[type].id_name : ""; }
inline constexpr GateLaunch gate_launch(uint8_t type) { return GATE_TABLE[type].launch; }      // type <= G_LAST
inline constexpr int gate_from_tag(uint32_t tag) { for (int t = 0; t <= G_LAST; t++) if (GATE_TABLE[t].tag == tag) return t; return -1; }

// ---- what follows from the table ----
// rows in enum order, and as many names in GL_GATE_LIST as rows: a new row without its list entry does not compile
constexpr bool gate_table_is_sound() {
    for (int t = 0; t <= G_LAST; t++) if (GATE_TABLE[t].type != t) return false;
    int names = 1;
    for (const char* s = GL_GATE_LIST; *s; s++) names += *s == ',';
    return names == G_LAST + 1;
}
static_assert(gate_table_is_sound(), "GATE_TABLE: rows in enum order, and GL_GATE_LIST naming every row");
constexpr unsigned max_gate_constraints() {
    unsigned m = 0;
    for (int t = 0; t <= G_LAST; t++)
        for (unsigned b = RANDOM_ACCESS_MIN_BITS; b <= RANDOM_ACCESS_MAX_BITS; b++) m = gate_num_constraints(t, b) > m ? gate_num_constraints(t, b) : m;
    return m;
}
}  // namespace glhost
// the widest gate (the PoseidonGate's 123): sizes the alpha-power table of the quotient kernels and the verifier's constraint buffer
constexpr unsigned GL_MAX_GATE_CONSTRAINTS = glhost::max_gate_constraints();
