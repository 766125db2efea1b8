// parser.cpp -- the .pbrt scene-file front end, text side: tokenizer, typed parameter lists and the directive chain, which
// calls the Api (api.h, api.cpp) directive by directive; and the two entry points that load a scene (scene.h).
//
// Behaviour restated from the reference (same directive and parameter names, defaults, "report and continue" policy):
//   tokenizer / parameter typing      src/core/parser.cpp:252-330,440-790
//   directive dispatch                src/core/parser.cpp:786-1090
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include "api.h"

namespace mipt {
namespace {

// ------------------------------------------------------------------ tokenizer
struct Tokenizer {
    std::string text, filename;
    size_t pos = 0;
    int line = 1;
    bool Next(std::string *tok, bool *quoted, std::string *err) {
        *quoted = false;
        while (pos < text.size()) {
            char ch = text[pos];
            if (ch == '\n') { ++line; ++pos; }
            else if (ch == ' ' || ch == '\t' || ch == '\r') ++pos;
            else if (ch == '#') { while (pos < text.size() && text[pos] != '\n') ++pos; }
            else break;
        }
        if (pos >= text.size()) return false;
        char ch = text[pos];
        if (ch == '"') {
            ++pos;
            std::string out;
            bool closed = false;
            while (pos < text.size()) {
                char c = text[pos];
                if (c == '"') { closed = true; break; }
                if (c == '\n') { *err = "premature EOL in string"; return false; }
                if (c == '\\' && pos + 1 < text.size()) {
                    ++pos;
                    char e = text[pos];
                    static const char kEscapes[] = "bfnrt\\'\"", kValues[] = "\b\f\n\r\t\\'\"";
                    const char *at = e ? strchr(kEscapes, e) : nullptr;
                    if (!at) { *err = "bad escaped character"; return false; }
                    out += kValues[at - kEscapes];
                } else
                    out += c;
                ++pos;
            }
            if (!closed) { *err = "premature EOF in string"; return false; }
            ++pos;
            *tok = out;
            *quoted = true;
            return true;
        }
        if (ch == '[' || ch == ']') { *tok = std::string(1, ch); ++pos; return true; }
        size_t start = pos;
        while (pos < text.size()) {
            char c = text[pos];
            if (c == ' ' || c == '\n' || c == '\t' || c == '\r' || c == '"' || c == '[' || c == ']') break;
            ++pos;
        }
        *tok = text.substr(start, pos - start);
        return true;
    }
};

double ParseNumber(const std::string &s, bool *ok) {  // parser.cpp:322-368
    *ok = true;
    if (s.size() == 1) {
        if (!(s[0] >= '0' && s[0] <= '9')) { *ok = false; return 0; }
        return s[0] - '0';
    }
    bool isInt = true;
    for (char c : s) if (!(c >= '0' && c <= '9')) isInt = false;
    char *end = nullptr;
    double val;
    if (isInt) val = double(strtol(s.c_str(), &end, 10));
    else val = strtof(s.c_str(), &end);  // Float == float
    if (val == 0 && end == s.c_str()) *ok = false;
    return val;
}

}  // namespace

// ReadFloatFile, src/core/floatfile.cpp:40-83 (including its habit of dropping a number that ends at end-of-file)
bool ReadFloatFile(const std::string &filename, std::vector<float> *values, Api *api) {
    FILE *f = fopen(filename.c_str(), "r");
    if (!f) { api->Err("Unable to open file \"" + filename + "\""); return false; }
    int c;
    bool inNumber = false;
    char curNumber[32];
    int curNumberPos = 0;
    int lineNumber = 1;
    while ((c = getc(f)) != EOF) {
        if (c == '\n') ++lineNumber;
        if (inNumber) {
            if (curNumberPos >= (int)sizeof(curNumber) - 1) { api->Err("Overflowed buffer for parsing number in file: " + filename); fclose(f); return false; }
            if (isdigit(c) || c == '.' || c == 'e' || c == '-' || c == '+') curNumber[curNumberPos++] = (char)c;
            else {
                curNumber[curNumberPos++] = '\0';
                values->push_back((float)atof(curNumber));
                inNumber = false;
                curNumberPos = 0;
            }
        } else {
            if (isdigit(c) || c == '.' || c == '-' || c == '+') { inNumber = true; curNumber[curNumberPos++] = (char)c; }
            else if (c == '#') {
                while ((c = getc(f)) != '\n' && c != EOF) {}
                ++lineNumber;
            } else if (!isspace(c))
                api->Warn("Unexpected text found at line " + std::to_string(lineNumber) + " of float file \"" + filename + "\"");
        }
    }
    fclose(f);
    return true;
}

namespace {

// Blackbody / BlackbodyNormalized, src/core/spectrum.cpp:1009-1034
void Blackbody(const float *lambda, int n, float T, float *Le) {
    if (T <= 0) { for (int i = 0; i < n; ++i) Le[i] = 0.f; return; }
    const float c = 299792458;
    const float h = 6.62606957e-34;
    const float kb = 1.3806488e-23;
    for (int i = 0; i < n; ++i) {
        float l = lambda[i] * 1e-9;
        float lambda5 = (l * l) * (l * l) * l;
        Le[i] = (2 * h * c * c) / (lambda5 * (std::exp((h * c) / (l * kb * T)) - 1));
    }
}
void BlackbodyNormalized(const float *lambda, int n, float T, float *Le) {
    Blackbody(lambda, n, T, Le);
    float lambdaMax = 2.8977721e-3 / T * 1e9;
    float maxL;
    Blackbody(&lambdaMax, 1, T, &maxL);
    for (int i = 0; i < n; ++i) Le[i] /= maxL;
}

// ------------------------------------------------------------------ parser
enum ParamType { PT_INT, PT_BOOL, PT_FLOAT, PT_POINT2, PT_VECTOR2, PT_POINT3, PT_VECTOR3, PT_NORMAL, PT_RGB, PT_XYZ,
                 PT_BLACKBODY, PT_SPECTRUM, PT_STRING, PT_TEXTURE, PT_UNKNOWN };

bool LookupType(const std::string &decl, ParamType *type, std::string *name) {  // parser.cpp:440-520
    size_t i = 0;
    auto skip = [&]() { while (i < decl.size() && (decl[i] == ' ' || decl[i] == '\t')) ++i; };
    skip();
    size_t ts = i;
    while (i < decl.size() && decl[i] != ' ' && decl[i] != '\t') ++i;
    std::string t = decl.substr(ts, i - ts);
    skip();
    size_t ns = i;
    while (i < decl.size() && decl[i] != ' ' && decl[i] != '\t') ++i;
    *name = decl.substr(ns, i - ns);
    if (t.empty() || name->empty()) return false;
    static const std::pair<const char *, ParamType> kTypes[] = {
        {"float", PT_FLOAT}, {"integer", PT_INT}, {"bool", PT_BOOL}, {"point2", PT_POINT2}, {"vector2", PT_VECTOR2},
        {"point3", PT_POINT3}, {"point", PT_POINT3}, {"vector3", PT_VECTOR3}, {"vector", PT_VECTOR3}, {"normal", PT_NORMAL},
        {"string", PT_STRING}, {"texture", PT_TEXTURE}, {"color", PT_RGB}, {"rgb", PT_RGB}, {"xyz", PT_XYZ},
        {"blackbody", PT_BLACKBODY}, {"spectrum", PT_SPECTRUM}};
    *type = PT_UNKNOWN;
    for (const auto &entry : kTypes) if (t == entry.first) *type = entry.second;
    return *type != PT_UNKNOWN;
}

struct Parser {
    Api *api;
    std::vector<Tokenizer> stack;
    bool hasUnget = false;
    std::string ungetTok;
    bool ungetQuoted = false;
    std::string error;

    bool Next(std::string *tok, bool *quoted) {
        if (hasUnget) { hasUnget = false; *tok = ungetTok; *quoted = ungetQuoted; return true; }
        while (!stack.empty()) {
            std::string err;
            if (stack.back().Next(tok, quoted, &err)) return true;
            if (!err.empty()) { error = stack.back().filename + ":" + std::to_string(stack.back().line) + ": " + err; return false; }
            stack.pop_back();
        }
        return false;
    }
    void Unget(const std::string &tok, bool quoted) { hasUnget = true; ungetTok = tok; ungetQuoted = quoted; }
    std::string Loc() { return stack.empty() ? std::string("<eof>") : stack.back().filename + ":" + std::to_string(stack.back().line); }
    bool Fail(const std::string &m) { if (error.empty()) error = Loc() + ": " + m; return false; }

    bool ParseParams(ParamSet *ps) {  // parser.cpp:707-780 + AddParam 520-705
        while (true) {
            std::string decl;
            bool q;
            if (!Next(&decl, &q)) return error.empty();
            if (!q) { Unget(decl, q); return true; }
            ParamType type = PT_UNKNOWN;
            std::string name;
            bool known = LookupType(decl, &type, &name);
            std::vector<double> nums;
            std::vector<std::string> strs;
            std::string val;
            bool vq;
            if (!Next(&val, &vq)) return Fail("premature EOF in parameter list");
            auto addVal = [&](const std::string &v, bool isq) -> bool {
                if (isq) {
                    if (!nums.empty()) return Fail("mixed string and numeric parameters");
                    strs.push_back(v);
                } else {
                    if (!strs.empty()) return Fail("mixed string and numeric parameters");
                    bool ok;
                    double dv = ParseNumber(v, &ok);
                    if (!ok) return Fail("\"" + v + "\": expected a number");
                    nums.push_back(dv);
                }
                return true;
            };
            if (!vq && val == "[") {
                while (true) {
                    if (!Next(&val, &vq)) return Fail("premature EOF in parameter list");
                    if (!vq && val == "]") break;
                    if (!addVal(val, vq)) return false;
                }
            } else if (!addVal(val, vq)) return false;
            if (!known) { api->Warn("Type of parameter \"" + decl + "\" is unknown"); continue; }
            bool wantString = (type == PT_STRING || type == PT_TEXTURE || type == PT_BOOL);
            if (type == PT_SPECTRUM && !strs.empty()) {  // AddSampledSpectrumFiles, paramset.cpp:171-207
                std::vector<Spectrum> v;
                for (const std::string &nm : strs) {
                    const std::string fn = api->AbsolutePath(nm);
                    auto cached = api->cachedSpectra.find(fn);
                    if (cached != api->cachedSpectra.end()) { v.push_back(cached->second); continue; }
                    std::vector<float> vals;
                    Spectrum sp(0.f);
                    if (!ReadFloatFile(fn, &vals, api))
                        api->Warn("Unable to read SPD file \"" + fn + "\".  Using black distribution.");
                    else {
                        if (vals.size() % 2) api->Warn("Extra value found in spectrum file \"" + fn + "\". Ignoring it.");
                        std::vector<float> wls, vv;
                        for (size_t j = 0; j < vals.size() / 2; ++j) { wls.push_back(vals[2 * j]); vv.push_back(vals[2 * j + 1]); }
                        if (!wls.empty()) sp = Spectrum::FromSampled(wls.data(), vv.data(), (int)wls.size());
                    }
                    api->cachedSpectra[fn] = sp;
                    v.push_back(sp);
                }
                ParamSet::Add(ps->spectra, name, v);
                continue;
            }
            if (wantString && strs.empty() && !nums.empty()) { api->Err("Expected string parameter value for \"" + name + "\""); continue; }
            if (!wantString && !strs.empty()) { api->Err("Expected numeric parameter value for \"" + name + "\""); continue; }
            size_t n = nums.size();
            auto f = [&](size_t i) { return (float)nums[i]; };
            switch (type) {
            case PT_INT: { std::vector<int> v(n); for (size_t i = 0; i < n; ++i) v[i] = int(nums[i]); ParamSet::Add(ps->ints, name, v); break; }
            case PT_BOOL: {
                std::vector<bool> v;
                for (auto &s : strs) {
                    if (s == "true") v.push_back(true);
                    else if (s == "false") v.push_back(false);
                    else { api->Warn("Value \"" + s + "\" unknown for Boolean parameter \"" + name + "\". Using \"false\"."); v.push_back(false); }
                }
                ParamSet::Add(ps->bools, name, v);
                break;
            }
            case PT_FLOAT: { std::vector<float> v(n); for (size_t i = 0; i < n; ++i) v[i] = f(i); ParamSet::Add(ps->floats, name, v); break; }
            case PT_POINT2: case PT_VECTOR2: {
                if (n % 2) api->Warn("Excess values given with point2 parameter \"" + name + "\". Ignoring last one of them.");
                std::vector<Vec2> v(n / 2);
                for (size_t i = 0; i < n / 2; ++i) { v[i].x = f(2 * i); v[i].y = f(2 * i + 1); }
                ParamSet::Add(ps->point2s, name, v);
                break;
            }
            case PT_POINT3: case PT_VECTOR3: case PT_NORMAL: {
                if (n % 3) api->Warn("Excess values given with parameter \"" + name + "\". Ignoring extra.");
                std::vector<Vec3> v(n / 3);
                for (size_t i = 0; i < n / 3; ++i) v[i] = Vec3(f(3 * i), f(3 * i + 1), f(3 * i + 2));
                ParamSet::Add(type == PT_POINT3 ? ps->point3s : (type == PT_VECTOR3 ? ps->vector3s : ps->normals), name, v);
                break;
            }
            case PT_RGB: case PT_XYZ: {
                if (n % 3) { api->Warn("Excess RGB values given with parameter \"" + name + "\"."); n -= n % 3; }
                std::vector<Spectrum> v;
                for (size_t i = 0; i < n / 3; ++i) {
                    float c[3] = {f(3 * i), f(3 * i + 1), f(3 * i + 2)};
                    // AddRGBSpectrum / AddXYZSpectrum use FromRGB / FromXYZ defaults (paramset.cpp:110-131)
                    v.push_back(type == PT_RGB ? Spectrum::FromRGB(c) : Spectrum::FromXYZ(c));
                }
                ParamSet::Add(ps->spectra, name, v);
                break;
            }
            case PT_SPECTRUM: {  // AddSampledSpectrum, paramset.cpp:152-169
                if (n % 2) { api->Warn("Non-even number of values given with sampled spectrum parameter \"" + name + "\". Ignoring extra."); n -= n % 2; }
                if (n == 0) { api->Err("empty sampled spectrum \"" + name + "\""); break; }
                std::vector<float> wl(n / 2), vv(n / 2);
                for (size_t i = 0; i < n / 2; ++i) { wl[i] = f(2 * i); vv[i] = f(2 * i + 1); }
                std::vector<Spectrum> v(1, Spectrum::FromSampled(wl.data(), vv.data(), (int)(n / 2)));
                ParamSet::Add(ps->spectra, name, v);
                break;
            }
            case PT_BLACKBODY: {  // AddBlackbodySpectrum, paramset.cpp:133-150: (temperature K, scale) pairs
                if (n % 2) { api->Warn("Excess value given with blackbody parameter \"" + name + "\". Ignoring extra one."); n -= n % 2; }
                std::vector<Spectrum> v;
                const int nCIESamples = 471;   // CIE_lambda = 360 .. 830 nm, spectrum.cpp:543
                std::vector<float> lambda(nCIESamples), le(nCIESamples);
                for (int i = 0; i < nCIESamples; ++i) lambda[i] = (float)(360 + i);
                for (size_t i = 0; i < n / 2; ++i) {
                    BlackbodyNormalized(lambda.data(), nCIESamples, f(2 * i), le.data());
                    v.push_back(f(2 * i + 1) * Spectrum::FromSampled(lambda.data(), le.data(), nCIESamples));
                }
                ParamSet::Add(ps->spectra, name, v);
                break;
            }
            case PT_STRING: ParamSet::Add(ps->strings, name, strs); break;
            case PT_TEXTURE:
                if (strs.size() == 1) ParamSet::Add(ps->textures, name, strs);
                else api->Err("Only one string allowed for \"texture\" parameter \"" + name + "\"");
                break;
            default: break;
            }
        }
    }

    bool ReadFloats(int n, float *out) {
        for (int i = 0; i < n; ++i) {
            std::string t; bool q;
            if (!Next(&t, &q) || q) return Fail("expected a number");
            bool ok;
            out[i] = (float)ParseNumber(t, &ok);
            if (!ok) return Fail("\"" + t + "\": expected a number");
        }
        return true;
    }
    bool ReadString(std::string *s) {
        bool q;
        if (!Next(s, &q) || !q) return Fail("expected quoted string");
        return true;
    }
    bool OpenFile(const std::string &path) {
        std::ifstream in(path, std::ios::binary);
        if (!in) return false;
        std::stringstream ss;
        ss << in.rdbuf();
        Tokenizer t;
        t.text = ss.str();
        t.filename = path;
        stack.push_back(std::move(t));
        return true;
    }

    bool Run();
};

bool Parser::Run() {
    Api &a = *api;
    std::string tok;
    bool quoted;
    auto needWorld = [&](const char *n) {
        if (a.state != Api::World) { a.Err(std::string("Scene description must be inside world block; \"") + n + "\" not allowed. Ignoring."); return false; }
        return true;
    };
    auto needOptions = [&](const char *n) {
        if (a.state != Api::Options) { a.Err(std::string("Options cannot be set inside world block; \"") + n + "\" not allowed.  Ignoring."); return false; }
        return true;
    };
    while (Next(&tok, &quoted)) {
        if (quoted) return Fail("unexpected string \"" + tok + "\"");
        if (tok == "AttributeBegin") { if (needWorld("AttributeBegin")) a.AttributeBegin(); }
        else if (tok == "AttributeEnd") { if (needWorld("AttributeEnd")) a.AttributeEnd(); }
        else if (tok == "TransformBegin") { if (needWorld("TransformBegin")) a.PushTransform('t'); }
        else if (tok == "TransformEnd") {
            if (!needWorld("TransformEnd")) continue;
            if (a.transformStack.empty() || a.pushKinds.back() != 't') { a.Err("Unmatched TransformEnd encountered. Ignoring it."); continue; }
            a.PopTransform();
        } else if (tok == "ActiveTransform") {   // api.cpp:1017-1034; the parser knows these three words (pbrtparse.y)
            std::string w; bool q;
            if (!Next(&w, &q)) return Fail("premature EOF");
            if (w == "All") a.activeBits = 3;
            else if (w == "StartTime") a.activeBits = 1;
            else if (w == "EndTime") a.activeBits = 2;
            else return Fail("ActiveTransform: expected All, StartTime or EndTime");
        } else if (tok == "Identity") a.ForActiveTransforms([](const Transform &) { return Transform(); });
        else if (tok == "Translate") { float v[3]; if (!ReadFloats(3, v)) return false; a.ConcatTransform(Translate(Vec3(v[0], v[1], v[2]))); }
        else if (tok == "Scale") { float v[3]; if (!ReadFloats(3, v)) return false; a.ConcatTransform(Scale(v[0], v[1], v[2])); }
        else if (tok == "Rotate") { float v[4]; if (!ReadFloats(4, v)) return false; a.ConcatTransform(Rotate(v[0], Vec3(v[1], v[2], v[3]))); }
        else if (tok == "LookAt") {
            float v[9]; if (!ReadFloats(9, v)) return false;
            bool degenerate;
            Transform la = LookAt(Vec3(v[0], v[1], v[2]), Vec3(v[3], v[4], v[5]), Vec3(v[6], v[7], v[8]), &degenerate);
            if (degenerate) a.Err("\"up\" vector and viewing direction passed to LookAt are pointing in the same direction.  Using the identity transformation.");
            a.ConcatTransform(la);
        } else if (tok == "Transform" || tok == "ConcatTransform") {
            std::string b; bool q;
            if (!Next(&b, &q) || b != "[") return Fail("expected [");
            float tr[16]; if (!ReadFloats(16, tr)) return false;
            if (!Next(&b, &q) || b != "]") return Fail("expected ]");
            Transform t(Matrix4x4(tr[0], tr[4], tr[8], tr[12], tr[1], tr[5], tr[9], tr[13], tr[2], tr[6], tr[10], tr[14],
                                  tr[3], tr[7], tr[11], tr[15]));
            if (tok == "Transform") a.ForActiveTransforms([&](const Transform &) { return t; });
            else a.ConcatTransform(t);
        } else if (tok == "CoordinateSystem") { std::string n; if (!ReadString(&n)) return false; a.namedCoordSys[n] = std::make_pair(a.ctm, a.ctmEnd); }
        else if (tok == "CoordSysTransform") {   // the whole pair, whatever the active bits say (api.cpp:1002-1015)
            std::string n; if (!ReadString(&n)) return false;
            if (a.namedCoordSys.count(n)) { a.ctm = a.namedCoordSys[n].first; a.ctmEnd = a.namedCoordSys[n].second; }
            else a.Warn("Couldn't find named coordinate system \"" + n + "\"");
        } else if (tok == "TransformTimes") {   // api.cpp:1036-1044
            float v[2]; if (!ReadFloats(2, v)) return false;
            if (!needOptions("TransformTimes")) continue;
            a.transformStart = v[0]; a.transformEnd = v[1];
        }
        else if (tok == "ReverseOrientation") { if (needWorld("ReverseOrientation")) a.gs.reverseOrientation = !a.gs.reverseOrientation; }
        else if (tok == "Include") {
            std::string fn; if (!ReadString(&fn)) return false;
            std::string path = (fn.size() && fn[0] == '/') ? fn : a.baseDir + "/" + fn;  // ResolveFilename (not AbsolutePath: no name is the directory here)
            if (!OpenFile(path)) a.Err("Couldn't open include file \"" + path + "\"");
        } else if (tok == "WorldBegin") {
            if (!needOptions("WorldBegin")) continue;
            a.state = Api::World;
            a.ctm = a.ctmEnd = Transform();
            a.activeBits = 3;
            a.namedCoordSys["world"] = std::make_pair(a.ctm, a.ctmEnd);
        } else if (tok == "WorldEnd") {
            if (!needWorld("WorldEnd")) continue;
            while (!a.gsStack.empty()) { a.Warn("Missing end to AttributeBegin"); a.gsStack.pop_back(); a.transformStack.pop_back(); }
            a.WorldEnd();
            a.state = Api::Options;
            return true;  // one render per file on this path
        } else if (tok == "ObjectBegin" || tok == "ObjectInstance") {
            std::string n; if (!ReadString(&n)) return false;
            if (!needWorld(tok.c_str())) continue;
            if (tok == "ObjectBegin") a.ObjectBegin(n); else a.ObjectInstance(n);
        } else if (tok == "ObjectEnd") { if (needWorld("ObjectEnd")) a.ObjectEnd(); }
        else if (tok == "MediumInterface") {
            std::string n; if (!ReadString(&n)) return false;
            std::string t2; bool q2;
            if (Next(&t2, &q2) && !q2) Unget(t2, q2);
            a.Warn("MediumInterface ignored: PathIntegrator does not handle media (path.cpp:122-123)");
        } else {
            // directives of the form:  Name "type" <params>
            static const char *named[] = {"Camera", "Film", "Sampler", "Accelerator", "Integrator", "PixelFilter", "Material",
                                          "MakeNamedMaterial", "NamedMaterial", "AreaLightSource", "LightSource", "Shape",
                                          "Texture", "MakeNamedMedium"};
            bool isNamed = false;
            for (const char *n : named) if (tok == n) isNamed = true;
            if (!isNamed) return Fail("unknown directive \"" + tok + "\"");
            std::string name;
            if (!ReadString(&name)) return false;
            std::string texType, texClass;
            if (tok == "Texture") { if (!ReadString(&texType) || !ReadString(&texClass)) return false; }
            ParamSet ps;
            if (tok != "NamedMaterial") { if (!ParseParams(&ps)) return false; }
            if (tok == "Camera") {
                if (!needOptions("Camera")) continue;
                a.cameraName = name; a.cameraParams = ps;
                a.cameraToWorld = Inverse(a.ctm);   // the pair of inverses (Inverse(TransformSet), api.cpp:179-184)
                a.cameraToWorldEnd = Inverse(a.ctmEnd);
                a.namedCoordSys["camera"] = std::make_pair(a.cameraToWorld, a.cameraToWorldEnd);
            } else if (tok == "Film") { if (needOptions("Film")) { a.filmName = name; a.filmParams = ps; } }
            else if (tok == "Sampler") { if (needOptions("Sampler")) { a.samplerName = name; a.samplerParams = ps; } }
            else if (tok == "Accelerator") { if (needOptions("Accelerator")) { a.accelName = name; a.accelParams = ps; } }
            else if (tok == "Integrator") { if (needOptions("Integrator")) { a.integratorName = name; a.integratorParams = ps; } }
            else if (tok == "PixelFilter") { if (needOptions("PixelFilter")) { a.filterName = name; a.filterParams = ps; } }
            else if (tok == "Material") { if (needWorld("Material")) a.gs.currentMaterial = a.NewMaterialInstance(name, ps); }
            else if (tok == "MakeNamedMaterial") {
                if (!needWorld("MakeNamedMaterial")) continue;
                a.WarnIfAnimated("MakeNamedMaterial");   // api.cpp:1287
                std::string matName = ps.FindOneString("type", "");
                if (matName == "") { a.Err("No parameter string \"type\" found in MakeNamedMaterial"); continue; }
                auto mi = a.NewMaterialInstance(matName, ps);
                if (a.gs.namedMaterials.count(name)) a.Warn("Named material \"" + name + "\" redefined.");
                a.gs.namedMaterials[name] = mi;
            } else if (tok == "NamedMaterial") {
                if (!needWorld("NamedMaterial")) continue;
                auto it = a.gs.namedMaterials.find(name);
                if (it == a.gs.namedMaterials.end()) { a.Err("NamedMaterial \"" + name + "\" unknown."); continue; }
                a.gs.currentMaterial = it->second;
            } else if (tok == "AreaLightSource") { if (needWorld("AreaLightSource")) { a.gs.areaLight = name; a.gs.areaLightParams = ps; } }
            else if (tok == "LightSource") a.LightSource(name, ps);
            else if (tok == "Shape") a.Shape(name, ps);
            else if (tok == "Texture") { if (needWorld("Texture")) a.Texture(name, texType, texClass, ps); }
            else if (tok == "MakeNamedMedium") { a.WarnIfAnimated("MakeNamedMedium"); a.Warn("MakeNamedMedium ignored: media are outside the hot-path scope"); }
        }
    }
    return error.empty();
}

HostScene *Load(Parser &p, Api &api, HostScene *scene, std::string *err) {
    bool ok = p.Run();
    if (!ok) { *err = p.error.empty() ? "parse error" : p.error; delete scene; return nullptr; }
    if (!api.worldEnded) { *err = "scene file has no WorldEnd"; delete scene; return nullptr; }
    return scene;
}

}  // namespace

HostScene *LoadSceneFile(const std::string &path, const LoadOverrides &ov, std::string *err) {
    HostScene *scene = new HostScene();
    Api api(scene, ov);
    size_t slash = path.find_last_of('/');
    api.baseDir = (slash == std::string::npos) ? "." : path.substr(0, slash);
    Parser p;
    p.api = &api;
    if (!p.OpenFile(path)) { *err = "Couldn't open scene file \"" + path + "\""; delete scene; return nullptr; }
    return Load(p, api, scene, err);
}

HostScene *LoadSceneString(const std::string &text, const std::string &baseDir, const LoadOverrides &ov, std::string *err) {
    HostScene *scene = new HostScene();
    Api api(scene, ov);
    api.baseDir = baseDir.empty() ? "." : baseDir;
    Parser p;
    p.api = &api;
    Tokenizer t;
    t.text = text;
    t.filename = "<string>";
    p.stack.push_back(std::move(t));
    return Load(p, api, scene, err);
}

}  // namespace mipt
