// tokenizer.h - host-side text front end of the semantic stage.
// Behavioural contract: /root/reference/bark.cpp:480-662 (utf8_len, strip_accents, bert_tokenize,
// bark_tokenize_input) including its quirks: no lower-casing, no CLS/SEP,
// at most n_max-1 word pieces, unknown bytes are skipped one at a time and force a "##" prefix.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace barkhip {

struct Vocab {
    std::unordered_map<std::string, int32_t> token_to_id;
    void build(const std::vector<std::string> & id_to_token);
};

// Latin-1 accented letters -> ASCII base letter (the 52 letters of bark.cpp:488-541).
std::string fold_accents(const std::string & text);

// Greedy longest-match WordPiece over regex-split words; writes at most n_max-1 ids.
int wordpiece_encode(const Vocab & vocab, const char * text, int32_t * out, int n_max, bool log_unknown);

struct PromptParams {
    int32_t block_size = 1024, text_encoding_offset = 10048, text_pad_token = 129595,
            semantic_pad_token = 10000, semantic_infer_token = 129599;
};
// 256 text slots (+offset, padded) | 256 semantic-history pads | infer token  -> 513 ids
std::vector<int32_t> build_semantic_prompt(const Vocab & vocab, const PromptParams & p, const char * text, bool log_unknown);

// Long-form text (rule C15s): the chunks of a text of any length as byte spans [begin, end) into it, each within the 256 text
// slots of a prompt.  Whitespace is space, \t, \n, \r, \f, \v; a word is a maximal run of other bytes; count(span) is wordpiece_encode of the span's
// bytes with n_max = 257 (256: over).  A word ends a SENTENCE if, with trailing closers (" ' ) ] } U+201D U+2019 U+00BB) stripped, its last byte is
// . ! ? or it ends in U+2026, or if the whitespace behind it holds a \n; it ends a CLAUSE if the stripped last byte is , ; : or the whole word is
// - U+2013 U+2014.  Budget B: max_tokens 0 -> 255 without merging (one sentence per chunk), 1 .. 255 -> max_tokens with greedy merging.
// From word s: E = the last word with count(s .. e) <= B for every e up to it (a single word over B is a chunk of its own).  E the last word: the
// chunk is s .. end (without merging the first sentence end in [s, E] still ends it).  Else the cut is the sentence end in [s, E] (the LAST with
// merging, the FIRST without), else the last clause end in [s, E], else E.  No word: no chunk.  Throws std::runtime_error for max_tokens outside
// 0 .. 255 and for more than kSplitMaxChunks chunks.
constexpr int kSplitMaxChunks = 64;
struct TextSpan { int32_t begin, end; };
std::vector<TextSpan> split_text(const Vocab & vocab, const std::string & text, int max_tokens);

}  // namespace barkhip
