// The proof-of-knowledge types of include/blsful_hip.hpp -- ProofCommitmentChallenge, ProofOfKnowledge, ProofOfKnowledgeTimestamp
// (reference src/proof_commitment.rs:256-261, src/proof_of_knowledge.rs:132-164, 287-326) -- on proofs that
// tests/test_cpp_pok_timestamp.py makes with the oracle and hands over as "key hex" lines: per orientation one valid proof, checked
// without a timeout, inside it and past it.
// Build: g++ -std=c++17 -I include tests/cpp/pok_timestamp_test.cpp -L agora-blsful_amd -lblsgpu   (needs a gfx950 device to run)
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
static void test_timestamp_proof(const std::map<std::string, std::string>& kat, const std::string& pre) {
  ProofOfKnowledgeTimestamp<C> pr{(SignatureSchemes)std::stoi(kat.at(pre + "scheme")), {}, {}, std::stoull(kat.at(pre + "t"))};
  PublicKey<C> pk;
  const Bytes u = unhex(kat.at(pre + "u")), v = unhex(kat.at(pre + "v")), k = unhex(kat.at(pre + "pk")), msg = unhex(kat.at(pre + "msg"));
  CHECK(u.size() == C::SIG_RAW && v.size() == C::SIG_RAW && k.size() == C::PK_RAW);
  std::memcpy(pr.u.data(), u.data(), C::SIG_RAW);
  std::memcpy(pr.v.data(), v.data(), C::SIG_RAW);
  std::memcpy(pk.raw.data(), k.data(), C::PK_RAW);
  const uint64_t now = std::stoull(kat.at("now")), timeout = std::stoull(kat.at("timeout"));
  CHECK(pr.verify(pk, msg).is_ok());                                                  // timeout None
  CHECK(pr.verify(pk, msg, timeout, now).is_ok());
  CHECK(pr.verify(pk, msg, timeout, pr.t + timeout).is_ok());                         // elapsed == timeout passes
  auto late = pr.verify(pk, msg, timeout, pr.t + timeout + 1);                        // timed out
  CHECK(late.is_err() && late.unwrap_err() == (BlsError{BlsError::Kind::InvalidProof, ""}));
  auto host = pr.verify(pk, msg, (uint64_t)1);                                        // this host's clock: the proof is years old
  CHECK(host.is_err() && host.unwrap_err().kind == BlsError::Kind::InvalidProof);
  auto future = pr.verify(pk, msg, timeout, pr.t - 1);
  CHECK(future.is_err() && future.unwrap_err().kind == BlsError::Kind::Runtime);
  Bytes other = msg;
  other.push_back(1);
  auto bad = pr.verify(pk, other);
  CHECK(bad.is_err() && bad.unwrap_err().kind == BlsError::Kind::InvalidProof);
  // the challenge, and the three-move form on it
  auto y = pr.challenge();
  CHECK(y.is_ok() && y.unwrap().to_le_bytes() == unhex(kat.at(pre + "y")));
  if (y.is_ok()) {
    ProofOfKnowledge<C> plain{pr.scheme, pr.u, pr.v};
    CHECK(plain.verify(pk, msg, y.unwrap()).is_ok());
    ProofCommitmentChallenge<C> y1 = y.unwrap();
    y1.le[0] ^= 1;
    CHECK(plain.verify(pk, msg, y1).is_err());
  }
  auto ch = ProofCommitmentChallenge<C>::from_hash(unhex(kat.at("seed")));
  CHECK(ch.is_ok() && ch.unwrap().to_le_bytes() == unhex(kat.at("seed_scalar")));
  if (ch.is_ok()) {
    Bytes be = ch.unwrap().to_be_bytes(), le = ch.unwrap().to_le_bytes();
    CHECK(be == Bytes(le.rbegin(), le.rend()));
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: %s <kat file>\n", argv[0]);
    return 2;
  }
  // no device: every call must fail loudly (there is no CPU path behind the mirror)
  {
    auto probe = ProofCommitmentChallenge<Bls12381G2Impl>::from_hash(Bytes{1, 2, 3});
    if (probe.is_err()) {
      std::printf("NO DEVICE: %s\n", probe.unwrap_err().message.c_str());
      return probe.unwrap_err().kind == BlsError::Kind::Runtime ? 3 : 1;
    }
  }
  auto kat = load(argv[1]);
  test_timestamp_proof<Bls12381G1Impl>(kat, "g1_");
  test_timestamp_proof<Bls12381G2Impl>(kat, "g2_");
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
