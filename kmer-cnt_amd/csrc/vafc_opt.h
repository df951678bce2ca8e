// vafc_opt.h -- command-line option scanner with the semantics of the
// reference's ketopt(s, argc, argv, permute = 1, ostr, longopts = 0)
// (ketopt.h:56-118), restated without rearranging argv:
//
//   - options may follow positional words: a word that does not start with
//     '-', and a lone "-", are positional wherever they stand;
//   - "--" ends the options: every later word is positional;
//   - any other word starting with "--" is one unknown option ('?');
//   - "-abc" is a cluster of short options; a letter that is not in ostr is
//     '?' and the cluster goes on;
//   - a letter followed by ':' in ostr takes an argument: the rest of its
//     word, or else the next word whatever it looks like; with no next word
//     the option comes back as ':' without an argument.
//
// vc_opt_next returns the option letter ('?' and ':' as above), or -1 when
// the words are used up; the positional words are then in `files`, in order.
#ifndef VAFC_OPT_H
#define VAFC_OPT_H

#include <string.h>

#include <vector>

struct VcOpt {
	int i = 1;                 // next word of argv
	int pos = 0;               // next letter of a cluster, 0 between words
	int opt = 0;               // the letter looked at last (ketopt_t.opt), 0 for a "--word"
	const char *arg = nullptr; // the option's argument, if any
	std::vector<const char *> files;
};

static inline int vc_opt_next(VcOpt &s, int argc, char *const argv[], const char *ostr)
{
	s.arg = nullptr;
	if (s.pos == 0) {
		while (s.i < argc && (argv[s.i][0] != '-' || argv[s.i][1] == '\0')) s.files.push_back(argv[s.i++]);
		if (s.i >= argc) return -1;
		if (argv[s.i][1] == '-') {
			if (argv[s.i][2] == '\0') {
				for (++s.i; s.i < argc; ++s.i) s.files.push_back(argv[s.i]);
				return -1;
			}
			s.opt = 0;
			++s.i;
			return '?';
		}
		s.pos = 1;
	}
	const char *word = argv[s.i];
	int opt = s.opt = (unsigned char)word[s.pos++];
	const char *p = strchr(ostr, opt);
	bool word_done = false;
	if (!p) {
		opt = '?';
	} else if (p[1] == ':') {
		if (word[s.pos] == '\0') {
			if (s.i < argc - 1) s.arg = argv[++s.i];
			else opt = ':';
		} else {
			s.arg = word + s.pos;
		}
		word_done = true;
	}
	if (word_done || word[s.pos] == '\0') {
		++s.i;
		s.pos = 0;
	}
	return opt;
}

#endif
