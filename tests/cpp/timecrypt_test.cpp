// TimeCryptCiphertext of include/blsful_hip.hpp (reference src/time_crypt_ciphertext.rs:38-50) on ciphertexts that
// tests/test_cpp_timecrypt.py seals with the oracle and hands over as "key hex" lines: per orientation a round trip, an empty w, a wrong
// signature, a mismatched scheme and a length beyond the frame.
// Build: g++ -std=c++17 -I include tests/cpp/timecrypt_test.cpp -L agora-blsful_amd -lblsgpu   (needs a gfx950 device to run)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>

#include "blsful_hip.hpp"

using namespace blsful;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    g_checks++;                                                                \
    if (!(cond)) {                                                             \
      g_failed++;                                                              \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
    }                                                                          \
  } while (0)

static Bytes unhex(const std::string& h) {
  Bytes b(h.size() / 2);
  for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
  return b;
}
static std::map<std::string, std::string> load(const char* path) {
  std::map<std::string, std::string> m;
  std::ifstream f(path);
  std::string line, k, v;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    v.clear();
    ss >> k >> v;
    m[k] = v;
  }
  return m;
}

template <class C>
static TimeCryptCiphertext<C> ciphertext(const std::map<std::string, std::string>& kat, const std::string& pre) {
  TimeCryptCiphertext<C> ct{{}, {}, unhex(kat.at(pre + "w")), (SignatureSchemes)std::stoi(kat.at(pre + "scheme"))};
  const Bytes u = unhex(kat.at(pre + "u")), v = unhex(kat.at(pre + "v"));
  CHECK(u.size() == C::PK_RAW && v.size() == 32);
  std::memcpy(ct.u.data(), u.data(), C::PK_RAW);
  std::memcpy(ct.v.data(), v.data(), 32);
  return ct;
}
template <class C>
static Signature<C> signature(const std::map<std::string, std::string>& kat, const std::string& key, SignatureSchemes scheme) {
  Signature<C> s{scheme, {}};
  const Bytes b = unhex(kat.at(key));
  CHECK(b.size() == C::SIG_RAW);
  std::memcpy(s.raw.data(), b.data(), C::SIG_RAW);
  return s;
}

template <class C>
static void test_time_lock(const std::map<std::string, std::string>& kat, const std::string& pre) {
  const auto ct = ciphertext<C>(kat, pre + "ct_");
  const auto sig = signature<C>(kat, pre + "sig", ct.scheme);
  auto plain = ct.decrypt(sig);                                                       // time_lock_works, tests/encryption.rs:66-87
  CHECK(plain.is_ok() && plain.unwrap().has_value() && *plain.unwrap() == unhex(kat.at(pre + "msg")));
  auto bad = ct.decrypt(signature<C>(kat, pre + "bad_sig", ct.scheme));
  CHECK(bad.is_ok() && !bad.unwrap().has_value());
  const SignatureSchemes other = ct.scheme == SignatureSchemes::Basic ? SignatureSchemes::MessageAugmentation : SignatureSchemes::Basic;
  auto bad_scheme = ct.decrypt(signature<C>(kat, pre + "sig", other));
  CHECK(bad_scheme.is_ok() && !bad_scheme.unwrap().has_value());
  auto empty = ciphertext<C>(kat, pre + "empty_").decrypt(sig);                       // an empty w: the empty message, decided by the check
  CHECK(empty.is_ok() && empty.unwrap().has_value() && empty.unwrap()->empty());
  auto beyond = ciphertext<C>(kat, pre + "beyond_").decrypt(sig);
  CHECK(beyond.is_ok() && !beyond.unwrap().has_value());
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: %s <kat file>\n", argv[0]);
    return 2;
  }
  // no device: the call must fail loudly (there is no CPU path behind the mirror)
  {
    TimeCryptCiphertext<Bls12381G2Impl> ct{{}, {}, Bytes(32), SignatureSchemes::Basic};
    auto probe = ct.decrypt(Signature<Bls12381G2Impl>{SignatureSchemes::Basic, {}});
    if (probe.is_err()) {
      std::printf("NO DEVICE: %s\n", probe.unwrap_err().message.c_str());
      return probe.unwrap_err().kind == BlsError::Kind::Runtime ? 3 : 1;
    }
    CHECK(!probe.unwrap().has_value());                                               // all-zero points: the identity signature
  }
  auto kat = load(argv[1]);
  test_time_lock<Bls12381G1Impl>(kat, "g1_");
  test_time_lock<Bls12381G2Impl>(kat, "g2_");
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
