// Stand-in for the reference's bison-generated Core/ArithmeticExpressionParser.hh (bison is not
// assumed).  Written from the one call site only, Configuration::resolveArithmeticExpressions
// (src/Core/Configuration.cc): a default-constructible ArithmeticExpressionParserDriver with
//     bool parse(const std::string&, double&)   and   std::string getLastError().
// It evaluates $[...] expressions of numbers, + - * / and parentheses by recursive descent; the
// scorer harness never puts such an expression into its configuration.
#pragma once
#include <cctype>
#include <cstdlib>
#include <string>

class ArithmeticExpressionParserDriver {
public:
    bool parse(const std::string& text, double& value) {
        s_ = text.c_str();
        error_.clear();
        double v = sum();
        skip();
        if (*s_ != '\0' && error_.empty())
            error_ = std::string(": unexpected '") + *s_ + "'";
        if (!error_.empty())
            return false;
        value = v;
        return true;
    }
    std::string getLastError() const {
        return error_;
    }

private:
    const char* s_ = "";
    std::string error_;

    void skip() {
        while (std::isspace(static_cast<unsigned char>(*s_)))
            ++s_;
    }
    double sum() {
        double v = product();
        for (skip(); *s_ == '+' || *s_ == '-'; skip()) {
            char   op = *s_++;
            double r  = product();
            v         = op == '+' ? v + r : v - r;
        }
        return v;
    }
    double product() {
        double v = unary();
        for (skip(); *s_ == '*' || *s_ == '/'; skip()) {
            char   op = *s_++;
            double r  = unary();
            v         = op == '*' ? v * r : v / r;
        }
        return v;
    }
    double unary() {
        skip();
        if (*s_ == '-') {
            ++s_;
            return -unary();
        }
        if (*s_ == '+') {
            ++s_;
            return unary();
        }
        if (*s_ == '(') {
            ++s_;
            double v = sum();
            skip();
            if (*s_ == ')')
                ++s_;
            else if (error_.empty())
                error_ = ": missing ')'";
            return v;
        }
        char*  end = nullptr;
        double v   = std::strtod(s_, &end);
        if (end == s_) {
            if (error_.empty())
                error_ = ": number expected";
            return 0;
        }
        s_ = end;
        return v;
    }
};
