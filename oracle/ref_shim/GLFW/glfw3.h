/* TEST INFRASTRUCTURE ONLY — stand-in for <GLFW/glfw3.h>: the names the
 * reference's camera.cuh mentions.  No window exists and no key is ever down. */
#pragma once

struct GLFWwindow;

#define GLFW_KEY_SPACE 32
#define GLFW_KEY_A 65
#define GLFW_KEY_D 68
#define GLFW_KEY_S 83
#define GLFW_KEY_W 87
#define GLFW_KEY_RIGHT 262
#define GLFW_KEY_LEFT 263
#define GLFW_KEY_DOWN 264
#define GLFW_KEY_UP 265
#define GLFW_KEY_LEFT_SHIFT 340

static inline int glfwGetKey(GLFWwindow *, int) { return 0; }
